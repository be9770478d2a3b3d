"""The traces of tests/test_breaker_edges_gpu.py and their premises, from the oracle alone (no GPU): DegradeSlot's
circuit breakers away from their comfortable parameters — statistic windows of 1 ms to 2^31 - 1 ms that are not aligned
with the second window, recovery times exact to the millisecond, longer than a batch or wrapped by the reference's int
arithmetic, thresholds met exactly, Math.round of the RT count, min_request_amount from 1 to 2^31 - 1, response times
longer than a batch, idle gaps in every breaker state, two breakers out of step, and the flow rule in front of them.

Every builder is a plain function of its arguments (fixed seeds) whose arrays are frozen; every reference a cached
replay through oracle.binding.LocalChain / LocalTraceGen that keeps the events, the results and every resource's state
after each batch; every premise a function of the oracle's answers. Premises that need transitions read `trace()`: the
hot resource's recorded events through a fresh LocalChain one at a time, with breaker() and breaker_stat() after each.

Sizes. Resource 0 is the hot one, resources 1..3 are cold (a hundred-odd entries a batch, walked by the short walker
under flags = 0). The device's k_seg hands a segment to the wave walker when it is longer than `short_max` records:
kShortMax = 256 (engine.h), or 64 once a batch holds 256 events per resource (api.cpp local_args, `lsplit`). Every
batch here gives the hot resource at least 600 records (entries and exits), above both; test_sizes asserts it.

Coverage. Every case whose breaker can open shows CLOSED -> OPEN, OPEN -> HALF_OPEN, HALF_OPEN -> CLOSED and HALF_OPEN
-> OPEN in the oracle, but for the cases in COVERAGE_EXCEPTIONS, each with its reason."""
import collections
import functools

import numpy as np
import pytest

from oracle.binding import LocalChain, LocalTraceGen, degrade_rule, local_rule
from sentinel_amd import abi

RT, ER, EC = abi.DEGRADE_RT, abi.DEGRADE_EXCEPTION_RATIO, abi.DEGRADE_EXCEPTION_COUNT
QPS, THREAD, NONE = abi.FLOW_GRADE_QPS, abi.FLOW_GRADE_THREAD, abi.FLOW_GRADE_NONE
CLOSED, OPEN, HALF_OPEN = 0, 1, 2
T0 = 1_700_000_000_437  # a multiple of no statistic window used here (test_sizes)
GAPS = [70_000, 30 * 3_600_000]
I31 = (1 << 31) - 1
MIN_HOT_RECORDS = 600

# rules: one sg_local_rule per resource; batches: (entries, rt, err, t_end) for LocalTraceGen.run
Case = collections.namedtuple("Case", "rules S interval batches marks")
# outs: per batch (events, results, snapshot); snapshot: per resource (second, borrow, minute, threads, breakers),
# breakers: per breaker (state, next_retry, stat_start, bad, total)
Reference = collections.namedtuple("Reference", "outs")
# the hot resource's events in order: ev, want, batch [n], st [n, n_breakers, 5] after each event
Trace = collections.namedtuple("Trace", "ev want batch st")


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


COLD = [local_rule(60.0, QPS, [degrade_rule(ER, 0.3, 1, 5, 700)]),
        local_rule(0.0, NONE, [degrade_rule(RT, 20, 1, 5, 300, 0.4), degrade_rule(EC, 4, 2, 2, 1000)]),
        local_rule(8.0, THREAD)]


def _rules(hot_flow, hot_breakers, n_cold=3):
    r = np.zeros(1 + n_cold, abi.LOCAL_RULE_DTYPE)
    r[0] = local_rule(hot_flow[0], hot_flow[1], hot_breakers)
    for i in range(n_cold):
        r[1 + i] = COLD[i]
    return _freeze(r)[0]


def uniform(lo, hi, err):
    """rt uniform in [lo, hi], errors with probability err."""
    return lambda rng, ts: (rng.integers(lo, hi + 1, len(ts)), rng.random(len(ts)) < err)


def choice(rts, err):
    return lambda rng, ts: (rng.choice(np.asarray(rts), len(ts)), rng.random(len(ts)) < err)


def mixture(share, lo, hi, err_fast, err_slow, fast=(0, 30)):
    """`share` of the entries take lo..hi ms (errors with err_slow), the rest fast[0]..fast[1] (err_fast)."""
    def draw(rng, ts):
        slow = rng.random(len(ts)) < share
        rt = np.where(slow, rng.integers(lo, hi + 1, len(ts)), rng.integers(fast[0], fast[1] + 1, len(ts)))
        return rt, rng.random(len(ts)) < np.where(slow, err_slow, err_fast)
    return draw


def _batch(rng, t, span, hot, draw, n_cold=3, cold_n=120, prio=0.0, multi=0.0, t_end=None):
    """`hot` entries of resource 0 at uniform times in [t, t + span) — with hot >= span one at every millisecond and
    the rest uniform (dense traffic) — and cold_n of each cold resource; rt and err of the hot entries from `draw`."""
    if hot >= span:
        ts_hot = np.sort(np.concatenate([t + np.arange(span), t + rng.integers(0, span, hot - span)]))
    else:
        ts_hot = np.sort(t + rng.integers(0, span, hot))
    rt_hot, err_hot = draw(rng, ts_hot - t)
    ts_cold = t + rng.integers(0, span, n_cold * cold_n)
    res_cold = np.repeat(np.arange(1, 1 + n_cold, dtype=np.uint32), cold_n)
    ts = np.concatenate([ts_hot, ts_cold])
    order = np.argsort(ts, kind="stable")
    n = len(ts)
    e = np.zeros(n, abi.LOCAL_EVENT_DTYPE)
    e["ts_ms"] = ts[order]
    e["resource"] = np.concatenate([np.zeros(len(ts_hot), np.uint32), res_cold])[order]
    cnt = np.ones(n, np.int32)
    m = rng.random(n) < multi
    cnt[m] = rng.integers(2, 5, int(m.sum()))
    e["count"] = cnt
    e["resource"] |= np.where((rng.random(n) < prio) & (e["resource"] == 0), np.uint32(abi.KEY_PRIO), np.uint32(0))
    rt = np.concatenate([rt_hot, rng.integers(0, 41, len(ts_cold))])[order].astype(np.int32)
    err = np.concatenate([err_hot, rng.random(len(ts_cold)) < 0.15])[order].astype(np.uint8)
    return _freeze(e, rt, err) + (int(t + span if t_end is None else t_end),)


def _steady(seed, breakers, draw, n_batches=3, span=2500, hot=None, t0=T0, flow=(0.0, NONE), S=2, interval=1000,
            marks=None, **kw):
    """n_batches back to back, each of `span` ms with `hot` entries of the hot resource (dense by default)."""
    rng = np.random.default_rng(seed)
    hot = span + span // 2 if hot is None else hot
    batches = tuple(_batch(rng, t0 + i * span, span, hot, draw, **kw) for i in range(n_batches))
    return Case(_rules(flow, breakers), S, interval, batches, marks)


def snapshot(ora, n):
    out = []
    for r in range(n):
        sec, bor, mnt = ora.dump(r)
        cbs = []
        for i in range(2):
            st, nr = ora.breaker(r, i)
            if st >= 0:
                cbs.append((st, nr) + ora.breaker_stat(r, i))
        out.append(_freeze(sec, bor, mnt) + (ora.threads(r), tuple(cbs)))
    return tuple(out)


def _chain(case):
    ora = LocalChain(case.S, case.interval, 500)
    ora.load_rules(case.rules)
    return ora


def replay(case):
    ora = _chain(case)
    gen = LocalTraceGen(ora)
    outs = []
    for ent, rt, err, t_end in case.batches:
        ev, want = gen.run(ent, rt, err, t_end)
        outs.append(_freeze(ev, want) + (snapshot(ora, len(case.rules)),))
    return Reference(tuple(outs))


def trace(case, ref, res=0):
    """The recorded events of `res` (no rule here reads another resource) through a fresh chain, one at a time."""
    ora = _chain(case)
    nb = int(case.rules["n_breakers"][res])
    evs, wants, bs = [], [], []
    for b, (ev, want, _) in enumerate(ref.outs):
        m = (ev["resource"] & abi.KEY_INDEX) == res
        evs.append(ev[m])
        wants.append(want[m])
        bs.append(np.full(int(m.sum()), b))
    ev, want, batch = np.concatenate(evs), np.concatenate(wants), np.concatenate(bs)
    st = np.zeros((len(ev), nb, 5), np.int64)
    got = np.zeros(len(ev), abi.LOCAL_RES_DTYPE)
    for i in range(len(ev)):
        got[i] = ora.decide(ev[i:i + 1])[0]
        for j in range(nb):
            st[i, j, :2] = ora.breaker(res, j)
            st[i, j, 2:] = ora.breaker_stat(res, j)
    assert np.array_equal(got, want), "the one-at-a-time replay differs from the batched one"
    return Trace(*_freeze(ev, want, batch, st))


# ------------------------------------------------------------------- reading a trace

def is_entry(tr):
    return tr.ev["kind"] == abi.LOCAL_ENTRY


def before(tr, j):
    """Breaker j's (state, next_retry, stat_start, bad, total) before each event (CLOSED, never started, at first)."""
    first = np.array([[CLOSED, 0, abi.INT64_MIN, 0, 0]], np.int64)
    return np.concatenate([first, tr.st[:-1, j]])


def transitions(tr, j):
    """{(from, to): count} over the events (a probe reverted within its own entry shows as OPEN -> OPEN)."""
    a, b = before(tr, j)[:, 0], tr.st[:, j, 0]
    m = a != b
    return collections.Counter(zip(a[m].tolist(), b[m].tolist()))


ALL_FOUR = [(CLOSED, OPEN), (OPEN, HALF_OPEN), (HALF_OPEN, CLOSED), (HALF_OPEN, OPEN)]


def covers(tr, nb):
    return any(all(transitions(tr, j)[x] > 0 for x in ALL_FOUR) for j in range(nb))


def probes(tr, j):
    """Indices of the entries that left breaker j HALF_OPEN: its probes."""
    return np.nonzero(is_entry(tr) & (before(tr, j)[:, 0] == OPEN) & (tr.st[:, j, 0] == HALF_OPEN))[0]


def trips(tr, j):
    """Indices of the exits that opened breaker j (from CLOSED or HALF_OPEN)."""
    return np.nonzero(~is_entry(tr) & (before(tr, j)[:, 0] != OPEN) & (tr.st[:, j, 0] == OPEN))[0]


def rolls(tr, j):
    """The distinct statistic windows breaker j lived in."""
    s = tr.st[:, j, 2]
    return np.unique(s[s != abi.INT64_MIN])


def bad_delta(tr, j):
    """Per exit: what it added to breaker j's bad count (None-like -1 where a HALF_OPEN -> CLOSED reset hides it)."""
    b, a = before(tr, j), tr.st[:, j]
    prev = np.where(b[:, 2] == a[:, 2], b[:, 3], 0)
    d = a[:, 3] - prev
    d[(b[:, 0] == HALF_OPEN) & (a[:, 0] == CLOSED)] = -1
    d[is_entry(tr)] = -1
    return d


# ------------------------------------------------------------------- A. statistic windows

STD = uniform(0, 40, 0.4)  # rt 0..40 (about half above 20), four exits in ten in error
A_CASES = {
    "stat1": dict(breakers=[degrade_rule(ER, 0.3, 1, 2, 1)], seed=11),
    "stat7_13_t0": dict(breakers=[degrade_rule(ER, 0.3, 1, 3, 7), degrade_rule(RT, 20, 1, 4, 13, 0.5)], seed=12, t0=0),
    "stat300_700": dict(breakers=[degrade_rule(RT, 20, 1, 5, 300, 0.5), degrade_rule(ER, 0.3, 1, 5, 700)], seed=13),
    "stat999": dict(breakers=[degrade_rule(ER, 0.3, 1, 5, 999)], seed=14),
    "stat1000_S5": dict(breakers=[degrade_rule(ER, 0.3, 1, 5, 1000)], seed=15, S=5, interval=500),
    "stat_i31": dict(breakers=[degrade_rule(ER, 0.3, 1, 5, I31)], seed=17),
}


@functools.lru_cache(maxsize=None)
def stat_case(name):
    if name == "stat60000":
        # 60 000: the first window ends 4 s into the trace (inside the second batch); the fourth batch comes a
        # minute later, in the window after the next
        rng = np.random.default_rng(16)
        t0 = T0 - T0 % 60_000 + 60_000 - 4_000 + 437
        starts = [t0, t0 + 2000, t0 + 4000, t0 + 66_000]
        batches = tuple(_batch(rng, t, 2000, 3000, STD) for t in starts)
        return Case(_rules((0.0, NONE), [degrade_rule(ER, 0.3, 1, 5, 60_000)]), 2, 1000, batches, None)
    return _steady(draw=STD, **A_CASES[name])


A_NAMES = list(A_CASES) + ["stat60000"]


def premise_stat(name, case, tr):
    nb = int(case.rules["n_breakers"][0])
    for j in range(nb):
        w = rolls(tr, j)
        ms = int(case.rules["breakers"][0][j]["stat_interval_ms"])
        assert (w % ms == 0).all()
        if name == "stat_i31":
            assert len(w) == 1, "the 2^31 - 1 ms window rolled"
        else:
            assert len(w) >= 3, f"breaker {j}: {len(w)} statistic windows"
        if name == "stat60000":
            spans = [len(np.unique(tr.batch[tr.st[:, j, 2] == x])) for x in w]
            assert max(spans) >= 2, "no 60 s window spans two batches"


# ------------------------------------------------------------------- B. recovery time

WRAP_NEG, WRAP_704 = 2_147_484, 4_294_968  # * 1000 as an int: -2147483296 and 704 (AbstractCircuitBreaker.java:54)
B_NAMES = ["tw1_dense", "tw10", "wrap_neg", "wrap_704"]


def java_int(x):
    return (x + (1 << 31)) % (1 << 32) - (1 << 31)


@functools.lru_cache(maxsize=None)
def recovery_case(name):
    if name == "tw1_dense":
        return _steady(21, [degrade_rule(ER, 0.3, 1, 5, 500)], STD)
    if name == "tw10":  # four batches of 3.5 s: a trip in the first, the probe 10 s later in the last
        return _steady(22, [degrade_rule(ER, 0.3, 10, 5, 500)], STD, n_batches=4, span=3500, hot=1500)
    if name == "wrap_neg":
        return _steady(23, [degrade_rule(ER, 0.3, WRAP_NEG, 5, 500)], STD, n_batches=2, span=2000)
    if name == "wrap_704":
        return _steady(24, [degrade_rule(ER, 0.3, WRAP_704, 5, 500)], STD)
    raise KeyError(name)


def premise_recovery(name, case, tr):
    b, ent, ts = before(tr, 0), is_entry(tr), tr.ev["ts_ms"]
    ok = tr.want["status"] == abi.LOCAL_PASS
    tp = trips(tr, 0)
    assert len(tp) >= 1
    if name == "tw1_dense":
        at = ent & (b[:, 0] == OPEN) & (ts == b[:, 1]) & ok & (tr.st[:, 0, 0] == HALF_OPEN)
        just_before = ent & (b[:, 0] == OPEN) & (ts == b[:, 1] - 1) & (tr.want["status"] == abi.LOCAL_BLOCK_DEGRADE)
        assert at.sum() >= 1 and just_before.sum() >= 1, (int(at.sum()), int(just_before.sum()))
        assert (tr.st[tp, 0, 1] - ts[tp] == 1000).all()
    elif name == "tw10":
        whole = [bool((b[tr.batch == k, 0] == OPEN).all() and (tr.st[tr.batch == k, 0, 0] == OPEN).all())
                 for k in range(len(case.batches))]
        assert any(whole), "no batch with the breaker OPEN from its first event to its last"
        p = probes(tr, 0)
        assert len(p) >= 1 and tr.batch[p[0]] > tr.batch[tp[0]] and tr.batch[p[0]] > whole.index(True)
        assert ts[p[0]] - ts[tp[0]] >= 10_000
    elif name == "wrap_neg":
        assert java_int(WRAP_NEG * 1000) == -2147483296
        assert (tr.st[tp, 0, 1] == ts[tp] - 2147483296).all() and (tr.st[tp, 0, 1] < ts[tp]).all()
        # the next flow-passing entry after every trip is the probe
        for i in tp:
            nxt = np.nonzero(ent & (np.arange(len(ts)) > i))[0]
            assert len(nxt) == 0 or tr.st[nxt[0], 0, 0] == HALF_OPEN
        assert not (tr.want["status"] == abi.LOCAL_BLOCK_DEGRADE)[b[:, 0] == OPEN].any()
    elif name == "wrap_704":
        assert java_int(WRAP_704 * 1000) == 704
        assert (tr.st[tp, 0, 1] - ts[tp] == 704).all()


# ------------------------------------------------------------------- C. thresholds met exactly

C_CASES = {
    # exceptionRatio 1.0 cannot be exceeded: never opens
    "er_1.0": dict(breakers=[degrade_rule(ER, 1.0, 1, 5, 500)], draw=uniform(0, 40, 0.97), seed=31, hot=1500),
    "er_0.0": dict(breakers=[degrade_rule(ER, 0.0, 1, 5, 500)], draw=uniform(0, 40, 0.05), seed=4),
    "er_0.25": dict(breakers=[degrade_rule(ER, 0.25, 1, 4, 200)], draw=uniform(0, 40, 0.22), seed=33),
    "er_0.3": dict(breakers=[degrade_rule(ER, 0.3, 1, 10, 200)], draw=uniform(0, 40, 0.27), seed=34),
    "ec_3": dict(breakers=[degrade_rule(EC, 3, 1, 1, 50)], draw=uniform(0, 40, 0.05), seed=35, hot=2500),
    "ec_2.5": dict(breakers=[degrade_rule(EC, 2.5, 1, 1, 50)], draw=uniform(0, 40, 0.04), seed=4, hot=2500),
    "rt_0.0": dict(breakers=[degrade_rule(RT, 35, 1, 5, 500, 0.0)], draw=uniform(0, 40, 0.0), seed=37),
    "rt_1.0": dict(breakers=[degrade_rule(RT, 4, 1, 1, 20, 1.0)], draw=uniform(0, 40, 0.0), seed=38),
    "rt_0.5": dict(breakers=[degrade_rule(RT, 20, 1, 4, 100, 0.5)], draw=uniform(0, 40, 0.0), seed=1),
}
C_NAMES = list(C_CASES)


@functools.lru_cache(maxsize=None)
def threshold_case(name):
    return _steady(**C_CASES[name])


def _met_exactly(tr, rule):
    """Exits that leave bad / total (or bad, for a count) exactly at the threshold with the breaker CLOSED before and
    after them and min_request_amount reached."""
    b, a = before(tr, 0), tr.st[:, 0]
    bad, total = a[:, 3].astype(np.float64), a[:, 4]
    ratio = rule["grade"] != EC
    thr = rule["slow_ratio_threshold"] if rule["grade"] == RT else rule["count"]
    with np.errstate(divide="ignore", invalid="ignore"):
        cur = bad * 1.0 / total if ratio else bad
    return np.nonzero(~is_entry(tr) & (b[:, 0] == CLOSED) & (a[:, 0] == CLOSED) & (cur == thr) &
                      (total >= rule["min_request_amount"]))[0]


def premise_threshold(name, case, tr):
    rule = case.rules["breakers"][0][0]
    blocked = tr.want["status"] == abi.LOCAL_BLOCK_DEGRADE
    tp = trips(tr, 0)
    closed_trips = tp[before(tr, 0)[tp, 0] == CLOSED]
    if name == "er_1.0":
        assert tr.st[:, 0, 3].max() > 50 and not blocked.any() and (tr.st[:, 0, 0] == CLOSED).all()
        # ... with windows in which every exit so far is an error: the ratio is 1.0 exactly and does not trip
        assert len(_met_exactly(tr, rule)) >= 1
        return
    if name in ("er_0.0", "rt_0.0"):
        # the ratio 0 is met exactly (no bad exit yet) with the amount reached; the first bad exit then trips
        assert len(_met_exactly(tr, rule)) >= 1
        assert (tr.st[closed_trips, 0, 3] == 1).any()
    elif name in ("er_0.25", "er_0.3", "rt_0.5"):
        met = _met_exactly(tr, rule)
        assert len(met) >= 1 and len(closed_trips) >= 1 and closed_trips.max() > met.min()
    elif name in ("ec_3", "ec_2.5"):
        # a window that ends with exactly floor(count) bad exits, CLOSED throughout
        want_bad = 3 if name == "ec_3" else 2
        st = tr.st[:, 0]
        last = np.nonzero(np.append(st[1:, 2] != st[:-1, 2], True))[0]  # the last event of each window
        full = [i for i in last if st[i, 3] == want_bad and
                (st[st[:, 2] == st[i, 2], 0] == CLOSED).all()]
        assert len(full) >= 1, f"no window ends CLOSED with {want_bad} bad exits"
        assert (tr.st[closed_trips, 0, 3] == want_bad + 1).all() and len(closed_trips) >= 1
    elif name == "rt_1.0":
        # the Double.compare(...) == 0 clause: every trip from CLOSED has bad == total; windows with a fast exit
        # among slow ones stay CLOSED
        assert len(closed_trips) >= 1 and (tr.st[closed_trips, 0, 3] == tr.st[closed_trips, 0, 4]).all()
        st = tr.st[:, 0]
        assert ((st[:, 0] == CLOSED) & (st[:, 3] > 0) & (st[:, 3] < st[:, 4])).any()


# ------------------------------------------------------------------- D. Math.round of the RT count

# count -> maxAllowedRt = Math.round(count) (ResponseTimeCircuitBreaker.java:52): floor(count + 0.5) done exactly, so
# the largest double below 0.5 gives 0; 1e30 saturates at Long.MAX_VALUE
D_CASES = {"0.5": (0.5, 1), "0.49999999999999994": (0.49999999999999994, 0), "10.5": (10.5, 11), "1e30": (1e30, None)}
D_NAMES = list(D_CASES)
D_SEEDS = {"0.5": 2, "0.49999999999999994": 1, "10.5": 1, "1e30": 44}


@functools.lru_cache(maxsize=None)
def round_case(name):
    count, max_rt = D_CASES[name]
    rts = list(range(0, 41)) if max_rt is None else [max(0, max_rt - 1), max_rt, max_rt, max_rt, max_rt + 1]
    return _steady(D_SEEDS[name], [degrade_rule(RT, count, 1, 10, 300, 0.2)], choice(rts, 0.0))


def premise_round(name, case, tr):
    _, max_rt = D_CASES[name]
    d = bad_delta(tr, 0)
    rt = tr.ev["ts_ms"] - tr.ev["create_ts"]
    seen = d >= 0
    if max_rt is None:
        assert seen.sum() > 1000 and (d[seen] == 0).all() and (tr.st[:, 0, 0] == CLOSED).all()
        return
    at, above = seen & (rt == max_rt), seen & (rt == max_rt + 1)
    assert at.sum() >= 50 and above.sum() >= 20, (int(at.sum()), int(above.sum()))
    assert (d[at] == 0).all(), f"rt == {max_rt} counted as slow"
    assert (d[above] == 1).all(), f"rt == {max_rt + 1} not counted as slow"


# ------------------------------------------------------------------- E. min_request_amount

E_MID = 60  # between the exits a 100 ms window sees in the slow phases (about 30) and the fast ones (about 200)
E_NAMES = ["min1", "min_i31", "min_mid"]


@functools.lru_cache(maxsize=None)
def amount_case(name):
    if name == "min1":
        return _steady(51, [degrade_rule(ER, 0.3, 1, 1, 100)], STD)
    if name == "min_i31":
        return _steady(52, [degrade_rule(ER, 0.3, 1, I31, 100)], STD)
    # alternating phases of 0.3 and 2 entries a millisecond, three in ten in error against a ratio of 0.2
    rng = np.random.default_rng(53)
    batches, t = [], T0
    for hot in (700, 4000, 700, 4000):
        batches.append(_batch(rng, t, 2000, hot, uniform(0, 40, 0.3)))
        t += 2000
    return Case(_rules((0.0, NONE), [degrade_rule(ER, 0.2, 1, E_MID, 100)]), 2, 1000, tuple(batches), None)


def premise_amount(name, case, tr):
    st = tr.st[:, 0]
    if name == "min_i31":
        assert (st[:, 0] == CLOSED).all() and st[:, 3].max() > 10
        return
    if name == "min1":
        tp = trips(tr, 0)
        assert (st[tp[before(tr, 0)[tp, 0] == CLOSED], 4] == 1).any(), "no trip on a window's first exit"
        return
    last = np.nonzero(np.append(st[1:, 2] != st[:-1, 2], True))[0]
    totals = st[last, 4]
    assert totals.min() < E_MID < totals.max(), (totals.min(), totals.max())
    quiet = [i for i in last if st[i, 4] < E_MID and st[i, 3] > 0.2 * st[i, 4] and st[i, 4] >= 10 and
             (st[st[:, 2] == st[i, 2], 0] == CLOSED).all()]
    assert len(quiet) >= 1, "no window over the ratio that stays CLOSED below the amount"
    tp = trips(tr, 0)
    assert (st[tp, 4] >= E_MID)[before(tr, 0)[tp, 0] == CLOSED].all() and (before(tr, 0)[tp, 0] == CLOSED).any()


# ------------------------------------------------------------------- F. long response times

F_SEED = 3


@functools.lru_cache(maxsize=None)
def long_rt_case():
    """Four batches of 1000 ms, recovery 1 s, maxAllowedRt 100, statistic windows of 500 ms. The first batch's entries
    take 101..300 ms: the trip comes with the fifth exit (about 110 ms in) and the exits of what passed before it
    arrive while the breaker is OPEN. The second batch's take 1500..3000 ms: the probe (about 1110 ms) is the only
    request out, HALF_OPEN from there over the boundary at 2000 until it comes back, slow. The third batch's are all
    blocked. In the last (which runs on to 4400 ms) six in ten take 0..5 ms, the others 101..150 ms: a fast probe
    closes the breaker and the slow share opens it again."""
    rng = np.random.default_rng(F_SEED)
    tail = mixture(0.4, 101, 150, 0.0, 0.0, fast=(0, 5))
    batches = (_batch(rng, T0, 1000, 1500, uniform(101, 300, 0.0)),
               _batch(rng, T0 + 1000, 1000, 1500, uniform(1500, 3000, 0.0)),
               _batch(rng, T0 + 2000, 1000, 1500, tail),
               _batch(rng, T0 + 3000, 1000, 1500, tail, t_end=T0 + 4400))
    return Case(_rules((0.0, NONE), [degrade_rule(RT, 100, 1, 5, 500, 0.2)]), 2, 1000, batches, None)


def premise_long_rt(case, tr):
    later = 0
    for i in probes(tr, 0):
        nxt = np.nonzero(tr.st[i:, 0, 0] != HALF_OPEN)[0]  # the first exit after the probe's entry ends HALF_OPEN
        if len(nxt) == 0:
            continue
        k = i + nxt[0]
        own = not is_entry(tr)[k] and tr.ev["create_ts"][k] == tr.ev["ts_ms"][i]  # ... here: the probe's own
        later += int(own and tr.batch[k] > tr.batch[i])
    assert later >= 1, "no probe whose exit arrives in a later batch"
    ends = [np.nonzero(tr.batch == b)[0][-1] for b in range(len(case.batches) - 1)]
    assert any(tr.st[i, 0, 0] == HALF_OPEN for i in ends), "HALF_OPEN is carried over no batch boundary"
    assert (~is_entry(tr) & (before(tr, 0)[:, 0] == OPEN)).sum() >= 10, "too few exits while OPEN"
    rt = (tr.ev["ts_ms"] - tr.ev["create_ts"])[~is_entry(tr)]
    assert rt.max() >= 1500, "no long response time came back"


# ------------------------------------------------------------------- G. idle gaps

G_STATES = ["open", "half_open", "closed"]
G_SEED = 1


@functools.lru_cache(maxsize=None)
def gap_case(state, gap):
    """A first batch of 1400 ms of entries that ends in `state` and runs on until its last exit (a batch may not
    span the gap), the gap, then two batches of 2 s with six exits in ten in error.
    open: recovery 10 s and every exit in error. half_open: recovery 1 s, every exit in error, and from 900 ms on
    entries that stay out for the gap and 600 ms more: all are blocked but the probe (about 1005..1030 ms), which
    comes back some 120 ms into the batch after the gap. closed: one exit in ten in error against a ratio of 0.5: the
    last window holds some of each."""
    rng = np.random.default_rng(G_SEED)
    tw = 10 if state == "open" else 1

    def first(rng, ts):
        if state == "closed":
            return rng.integers(0, 41, len(ts)), rng.random(len(ts)) < 0.1
        rt = np.where(ts >= 900, gap + 600, rng.integers(0, 21, len(ts))) if state == "half_open" else \
            rng.integers(0, 21, len(ts))
        return rt, np.ones(len(ts), bool)
    t1 = T0 + 1500 + gap
    batches = (_batch(rng, T0, 1400, 2100, first, t_end=T0 + 1400 + 100),
               _batch(rng, t1, 2000, 3000, uniform(0, 40, 0.6)),
               _batch(rng, t1 + 2000, 2000, 3000, uniform(0, 40, 0.6)))
    return Case(_rules((0.0, NONE), [degrade_rule(ER, 0.5, tw, 5, 700)]), 2, 1000, batches, None)


def premise_gap(state, gap, case, tr):
    end0 = np.nonzero(tr.batch == 0)[0][-1]
    st, nr, start, bad, total = tr.st[end0, 0]
    first_entry = np.nonzero((tr.batch == 1) & is_entry(tr))[0][0]
    assert tr.ev["ts_ms"][first_entry] - tr.ev["ts_ms"][end0] >= gap
    for k in range(len(case.batches)):
        assert np.ptp(tr.ev["ts_ms"][tr.batch == k]) < 5000, "a batch spans the gap"
    if state == "open":
        assert st == OPEN and nr < tr.ev["ts_ms"][first_entry] and tr.st[first_entry, 0, 0] == HALF_OPEN
    elif state == "half_open":
        assert st == HALF_OPEN and tr.want["status"][first_entry] == abi.LOCAL_BLOCK_DEGRADE
        back = np.nonzero(~is_entry(tr) & (tr.batch == 1))[0][0]  # the probe's exit, the gap and 600 ms later
        assert tr.ev["ts_ms"][back] - tr.ev["create_ts"][back] == gap + 600 and tr.st[back, 0, 0] == OPEN
        assert (tr.st[end0:back, 0, 0] == HALF_OPEN).all()
    else:
        assert st == CLOSED and 0 < bad < total
        later = ~is_entry(tr) & (np.arange(len(tr.ev)) > first_entry)  # the window is rolled by the exits
        assert tr.st[later, 0, 2].min() > start, "the window before the gap is still counted"


# ------------------------------------------------------------------- H. two breakers out of step

H_ORDERS = ["1s_3s", "3s_1s"]
H_SEEDS = {"1s_3s": 81, "3s_1s": 9}


@functools.lru_cache(maxsize=None)
def two_case(order):
    """An RT breaker (maxAllowedRt 20, windows of 300 ms) and an exception-ratio breaker (windows of 700 ms) with
    recovery times of 1 s and 3 s, in both orders. Fifteen entries in a hundred take 2200..3000 ms and end in error,
    the others 0..40 ms without: the errors of what an open breaker let in before it opened arrive seconds later, so
    the second breaker can open while the first is OPEN, and later than it."""
    rt = lambda tw: degrade_rule(RT, 20, tw, 5, 300, 0.4)  # noqa: E731
    er = lambda tw: degrade_rule(ER, 0.5, tw, 3, 700)      # noqa: E731
    brk = [rt(1), er(3)] if order == "1s_3s" else [rt(3), er(1)]
    return _steady(H_SEEDS[order], brk, mixture(0.15, 2200, 3000, 0.0, 1.0, fast=(0, 40)), n_batches=4,
                   span=2500, hot=3000)


def premise_two(order, case, tr):
    s0, s1 = tr.st[:, 0], tr.st[:, 1]
    ts = tr.ev["ts_ms"]
    assert ((s0[:, 0] == OPEN) & (s1[:, 0] == OPEN) & (s0[:, 1] != s1[:, 1])).any(), "never both OPEN, out of step"
    b0 = before(tr, 0)
    reverted = is_entry(tr) & (b0[:, 0] == OPEN) & (s0[:, 0] == OPEN) & (s0[:, 1] <= ts) & (s1[:, 0] == OPEN) & \
        (s1[:, 1] > ts) & (tr.want["status"] == abi.LOCAL_BLOCK_DEGRADE)
    assert reverted.sum() >= 1, "no probe of the first breaker reverted by the second"
    # an exit that finds one breaker HALF_OPEN (and decides its probe) and the other CLOSED (and is counted there)
    b1 = before(tr, 1)
    half_closed = ~is_entry(tr) & (((b0[:, 0] == HALF_OPEN) & (b1[:, 0] == CLOSED)) |
                                   ((b1[:, 0] == HALF_OPEN) & (b0[:, 0] == CLOSED)))
    assert half_closed.any(), "never one HALF_OPEN beside one CLOSED and counting"


# ------------------------------------------------------------------- I. the flow rule in front

I_NAMES = ["low_qps", "prio", "thread", "no_flow", "saturated"]


I_SEEDS = {"low_qps": 1, "prio": 7, "thread": 2, "no_flow": 94, "saturated": 2}


@functools.lru_cache(maxsize=None)
def flow_case(name):
    er = [degrade_rule(ER, 0.3, 1, 5, 500)]
    seed = I_SEEDS[name]
    if name == "low_qps":
        # 20 QPS over a second window of (2, 2000), 1500 entries a second, min_request_amount 30: the 40 passes of a
        # window come at its start, the trip follows once 30 of them have left, and a second later the window is
        # still full. (Nothing passes while the breaker is OPEN: under (2, 1000), or with a trip before the window
        # is full, the window has room again at next_retry and the first entry there is the probe.)
        return _steady(seed, [degrade_rule(ER, 0.3, 1, 30, 500)], uniform(0, 40, 0.5), flow=(20.0, QPS), n_batches=4,
                       interval=2000)
    if name == "prio":       # one entry in a hundred prioritized: it occupies the next window, OPEN breaker or not
        return _steady(seed, er, uniform(0, 40, 0.4), flow=(100.0, QPS), prio=0.01, multi=0.1, n_batches=4)
    if name == "thread":
        return _steady(seed, er, uniform(0, 40, 0.25), flow=(20.0, THREAD), multi=0.1)
    if name == "no_flow":
        return _steady(seed, er, STD, multi=0.1)
    if name == "saturated":  # 4000 entries a second against 50 QPS, none prioritized: dead periods
        return _steady(seed, er, uniform(0, 40, 0.5), flow=(50.0, QPS), n_batches=4, span=1000, hot=4000, multi=0.1)
    raise KeyError(name)


def premise_flow(name, case, tr):
    b, ent, ts, status = before(tr, 0), is_entry(tr), tr.ev["ts_ms"], tr.want["status"]
    if name == "low_qps":
        late = 0
        for i in probes(tr, 0):
            first = np.nonzero(ent & (ts >= b[i, 1]) & (np.arange(len(ts)) <= i) & (b[:, 0] == OPEN) &
                               (b[:, 1] == b[i, 1]))[0][0]
            late += int(first < i and status[first] == abi.LOCAL_BLOCK_FLOW and ts[first] < ts[i])
        assert late >= 1, "every probe is the first entry at or after next_retry"
    if name == "saturated":
        n_pass = (status == abi.LOCAL_PASS).sum()
        assert (status == abi.LOCAL_BLOCK_FLOW).sum() > 10 * n_pass and n_pass > 3 * 50
        assert (ent & (b[:, 0] == OPEN)).sum() >= 1000 and not (tr.ev["resource"] & abi.KEY_PRIO).any()
    if name == "prio":
        assert (ent & (b[:, 0] == OPEN) & (status == abi.LOCAL_PASS_WAIT)).sum() >= 5, "no PASS_WAIT while OPEN"
    if name == "thread":
        assert (status == abi.LOCAL_BLOCK_FLOW).sum() >= 50 and (status == abi.LOCAL_BLOCK_DEGRADE).sum() >= 50
    if name == "no_flow":
        assert not (status == abi.LOCAL_BLOCK_FLOW).any()


# ------------------------------------------------------------------- every case, by name

COVERAGE_EXCEPTIONS = {
    "tw10": "recovery 10 s in a trace of 14 s: one probe",
    "er_1.0": "an exception ratio of 1.0 cannot be exceeded: never opens",
    "round_1e30": "no response time is above Long.MAX_VALUE: never opens",
    "min_i31": "2^31 - 1 exits never arrive in one window: never opens",
    "gap_open_70000": "recovery 10 s: one probe after the gap",
    "gap_open_108000000": "recovery 10 s: one probe after the gap",
}

CASES = {}
for _n in A_NAMES:
    CASES[_n] = (functools.partial(stat_case, _n), functools.partial(premise_stat, _n))
for _n in B_NAMES:
    CASES[_n] = (functools.partial(recovery_case, _n), functools.partial(premise_recovery, _n))
for _n in C_NAMES:
    CASES[_n] = (functools.partial(threshold_case, _n), functools.partial(premise_threshold, _n))
for _n in D_NAMES:
    CASES["round_" + _n] = (functools.partial(round_case, _n), functools.partial(premise_round, _n))
for _n in E_NAMES:
    CASES[_n] = (functools.partial(amount_case, _n), functools.partial(premise_amount, _n))
CASES["long_rt"] = (long_rt_case, premise_long_rt)
for _s in G_STATES:
    for _g in GAPS:
        CASES[f"gap_{_s}_{_g}"] = (functools.partial(gap_case, _s, _g), functools.partial(premise_gap, _s, _g))
for _n in H_ORDERS:
    CASES["two_" + _n] = (functools.partial(two_case, _n), functools.partial(premise_two, _n))
for _n in I_NAMES:
    CASES["flow_" + _n] = (functools.partial(flow_case, _n), functools.partial(premise_flow, _n))
NAMES = list(CASES)
FULL_CHAIN = ["wrap_neg", "wrap_704", "long_rt", "two_1s_3s", "two_3s_1s"]
PIPELINED = "long_rt"


def case(name):
    return CASES[name][0]()


@functools.lru_cache(maxsize=None)
def reference(name):
    return replay(case(name))


@functools.lru_cache(maxsize=None)
def case_trace(name):
    return trace(case(name), reference(name))


def premise(name):
    c, tr = case(name), case_trace(name)
    CASES[name][1](c, tr)
    nb = int(c.rules["n_breakers"][0])
    if name in COVERAGE_EXCEPTIONS:
        assert not covers(tr, nb), f"{name} is no exception any more"
    else:
        assert covers(tr, nb), f"{name}: transitions {[dict(transitions(tr, j)) for j in range(nb)]}"


@pytest.mark.parametrize("name", NAMES)
def test_premises(name):
    premise(name)


@pytest.mark.parametrize("name", NAMES)
def test_sizes(name):
    c, ref = case(name), reference(name)
    assert 2 <= len(c.batches) <= 4 and 3 <= len(c.rules) <= 6
    for (ent, _, _, _), (ev, _, _) in zip(c.batches, ref.outs):
        assert ((ent["resource"] & abi.KEY_INDEX) == 0).sum() <= 4000
        assert ((ev["resource"] & abi.KEY_INDEX) == 0).sum() >= MIN_HOT_RECORDS
    t_first = int(c.batches[0][0]["ts_ms"][0])
    for brk in c.rules["breakers"][0][:int(c.rules["n_breakers"][0])]:
        assert name == "stat7_13_t0" or brk["stat_interval_ms"] == 1 or t_first % int(brk["stat_interval_ms"]) != 0


def test_coverage_in_a_and_e():
    """Each of the four transitions at least once in at least one statistic-window case and one amount case."""
    assert any(covers(case_trace(n), int(case(n).rules["n_breakers"][0])) for n in A_NAMES)
    assert any(covers(case_trace(n), 1) for n in E_NAMES)
