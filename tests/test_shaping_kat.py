"""The oracle's WarmUpController / WarmUpRateLimiterController (oracle/sentinel_oracle.c, through
oracle.binding.Controller) against the independent model of tests/shaping_ref.py, away from cold factor 3: the same
seeded call sequences into both, equal results and equal {storedTokens, lastFilledTime, latestPassedTime} after every
call, over counts from fractions below the cold factor to 2^31, warm-up periods of 1..60 s and cold factors 2..10;
the model's own branch counters say what the drive reached. Constructor anchors computed by hand."""
import collections
import functools
import math

import numpy as np
import pytest

import shaping_ref as ref
from oracle.binding import Controller
from sentinel_amd import abi

WU, WRL = abi.CONTROL_WARM_UP, abi.CONTROL_WARM_UP_RATE_LIMITER
COUNTS = [0.0, 0.5, 1.0, 2.0, 2.9, 7.5, 20.0, 33.3, 100.0, 333.3, 1e5, 3e8, 1e9, 2.0 ** 31]
WARM_UP_SEC = [1, 3, 10, 60]
COLD = [2, 3, 4, 5, 10]
STARTS = [0, 999, 1_700_000_000_437]
CALLS = 400
MIN_VISITS = 1000


def _pair(count, warm, cold, behavior, visits=None, max_q=500):
    ora = Controller(count, warm, cold, behavior=behavior, max_queueing_ms=max_q)
    if behavior == WU:
        return ora, ref.WarmUpController(count, warm, cold, visits)
    return ora, ref.WarmUpRateLimiterController(count, warm, max_q, cold, visits)


def _drive(rng, count, start):
    """CALLS calls (now, passQps, previousPassQps, acquireCount): time steps of 0 ms, within a second, of a few seconds
    and up to 1e8 ms; rates around count / coldFactor and count (fractional, as StatisticNode.passQps() is at
    sampleCount 2 or interval 3000), idle seconds among them; acquire counts of 1, a few, and up to 2^30."""
    step = rng.choice(4, CALLS, p=[0.15, 0.45, 0.3, 0.1])
    dt = np.where(step == 0, 0, np.where(step == 1, rng.integers(1, 1000, CALLS),
                  np.where(step == 2, rng.integers(1000, 6000, CALLS), rng.integers(6000, 100_000_001, CALLS))))
    now = start + np.cumsum(dt)
    scale = min(max(count, 1.0), 1e6)
    qps = rng.random((2, CALLS)) * scale * rng.choice([0.0, 0.1, 0.4, 1.2, 3.0], (2, CALLS))
    qps = np.where(rng.random((2, CALLS)) < 0.5, np.floor(qps), qps)
    acq = np.where(rng.random(CALLS) < 0.8, 1, np.where(rng.random(CALLS) < 0.7, rng.integers(2, 8, CALLS),
                                                        rng.integers(8, (1 << 30) + 1, CALLS)))
    return now.tolist(), qps[0].tolist(), qps[1].tolist(), acq.tolist()


@functools.lru_cache(maxsize=None)
def _grid_visits():
    """Runs the grid once (both tests below read it): the number of calls and the model's branch visits."""
    visits = collections.Counter()
    calls = 0
    for ci, count in enumerate(COUNTS):
        for warm in WARM_UP_SEC:
            for cold in COLD:
                for behavior in (WU, WRL):
                    rng = np.random.default_rng([ci, warm, cold, behavior])
                    ora, mod = _pair(count, warm, cold, behavior, visits)
                    what = f"count {count} warmUp {warm} cold {cold} behavior {behavior}"
                    assert (ora.warning_token, ora.max_token) == (mod.warning_token, mod.max_token), what
                    now, pq, vq, acq = _drive(rng, count, STARTS[(ci + warm + cold) % len(STARTS)])
                    for i in range(CALLS):
                        if behavior == WU:
                            want = mod.can_pass(now[i], pq[i], vq[i], acq[i])
                            got = ora.warm_can_pass(now[i], pq[i], vq[i], acq[i])
                        else:
                            want = mod.can_pass(now[i], vq[i], acq[i])
                            got = ora.warm_rl_can_pass(now[i], vq[i], acq[i])
                        assert got == want and ora.state().tolist() == mod.state(), (
                            f"{what}, call {i} (now {now[i]} passQps {pq[i]} previous {vq[i]} acquire {acq[i]}): "
                            f"oracle {got} {ora.state().tolist()} vs model {want} {mod.state()}")
                    calls += CALLS
    return calls, visits


def test_oracle_equals_model_over_the_grid():
    calls, _ = _grid_visits()
    assert calls == len(COUNTS) * len(WARM_UP_SEC) * len(COLD) * 2 * CALLS >= 208_000


def test_the_drive_reaches_every_branch():
    _, visits = _grid_visits()
    print({b: visits[b] for b in ref.BRANCHES})
    for b in ref.BRANCHES:
        assert visits[b] >= MIN_VISITS, f"branch {b}: {visits[b]} visits"


# ---- constructor anchors, by hand (WarmUpController.java:95, :99, :104)

def _both(count, warm, cold, behavior=WU):
    ora, mod = _pair(count, warm, cold, behavior)
    assert (ora.warning_token, ora.max_token) == (mod.warning_token, mod.max_token)
    return ora, mod


def test_fractional_count_cold_2():
    ora, mod = _both(7.5, 3, 2)
    assert ora.warning_token == 22                 # (int)22.5 / 1
    assert ora.max_token == 22 + 15                # + (int)(6 * 7.5 / 3.0)
    assert mod.slope == 1.0 / 7.5 / 15


def test_fractional_count_cold_10():
    ora, mod = _both(7.5, 3, 10)
    assert ora.warning_token == 2                  # 22 / 9
    assert ora.max_token == 2 + 4                  # + (int)(45 / 11.0 = 4.09..)
    assert mod.slope == 9.0 / 7.5 / 4
    t = 1_700_000_000_000
    ora.warm_can_pass(t, 0, 0)                     # the first sync fills to maxToken
    mod.can_pass(t, 0, 0)
    assert ora.state().tolist() == mod.state() == [6, t, -1]
    # (int)7.5 / 10 == 0: no refill above the warning line, whatever the rate; - previousPassQps
    ora.warm_can_pass(t + 5000, 0, 0)
    mod.can_pass(t + 5000, 0, 0)
    assert ora.state().tolist() == mod.state() == [6, t + 5000, -1]
    ora.warm_can_pass(t + 6000, 0, 3)
    mod.can_pass(t + 6000, 0, 3)
    assert ora.state().tolist() == mod.state() == [3, t + 6000, -1]


def test_no_tokens_at_all():
    """warningToken == maxToken == 0: slope = 2 / 0.5 / 0 is infinite, aboveToken * slope = 0 * inf is NaN, and so is
    the warning QPS: `passQps + acquireCount <= NaN` blocks every WarmUp entry; Math.round(NaN) == 0 costs the
    WarmUpRateLimiter nothing and it passes every entry."""
    ora, mod = _both(0.5, 1, 3)
    assert (ora.warning_token, ora.max_token) == (0, 0)
    assert mod.slope == math.inf
    ora_rl, mod_rl = _both(0.5, 1, 3, WRL)
    t = 1_700_000_000_000
    for i in range(5):
        assert ora.warm_can_pass(t + 400 * i, 0, 0) is False and mod.can_pass(t + 400 * i, 0, 0) is False
        assert ora_rl.warm_rl_can_pass(t + 400 * i, 0) == mod_rl.can_pass(t + 400 * i, 0) == (True, 0)
    assert ora_rl.state().tolist() == mod_rl.state() == [0, t + 1000, t + 1600]


def test_count_zero():
    """count 0 (FlowRuleUtil.isValidRule accepts it): (2.0 / 0.0) / 0 is infinite; the same NaN."""
    ora, mod = _both(0.0, 10, 3)
    assert (ora.warning_token, ora.max_token) == (0, 0) and mod.slope == math.inf
    assert ora.warm_can_pass(5000, 0, 0) is False and mod.can_pass(5000, 0, 0) is False
    ora_rl, mod_rl = _both(0.0, 10, 3, WRL)
    assert ora_rl.warm_rl_can_pass(5000, 0, 1 << 30) == mod_rl.can_pass(5000, 0, 1 << 30) == (True, 0)


def test_int_max_and_wrap():
    """count 3e8, warmUp 10: (int)3e9 saturates at INT_MAX, / 2; + (int)(20 * 3e8 / 4.0) wraps negative. coolDownTokens
    then returns the negative maxToken and syncToken clamps the bucket to 0 every second."""
    ora, mod = _both(3e8, 10, 3)
    assert ora.warning_token == 2147483647 // 2 == 1073741823
    assert ora.max_token == 1073741823 + 1_500_000_000 - (1 << 32) == -1721225473
    assert mod.slope == 2.0 / 3e8 / float(-1721225473 - 1073741823 + (1 << 32))   # the int difference wraps back
    t = 1_700_000_000_000
    for i in range(4):
        assert ora.warm_can_pass(t + 700 * i, 5, 7) == mod.can_pass(t + 700 * i, 5, 7)
        assert ora.state().tolist() == mod.state() and mod.state()[0] == 0


@pytest.mark.parametrize("cold", [1, 0, -3])
def test_cold_factor_at_most_1(cold):
    """construct refuses it (:85-87); SentinelConfig.coldFactor() never hands it over (SentinelConfig.java:224-239:
    <= 1 becomes the default 3), which is what the oracle's entry points do."""
    with pytest.raises(ValueError):
        ref.WarmUpController(20.0, 3, cold)
    ora, mod = Controller(20.0, 3, cold), ref.WarmUpController(20.0, 3, 3)
    assert (ora.warning_token, ora.max_token) == (mod.warning_token, mod.max_token) == (30, 60)


def test_math_round_ties_go_up():
    """Math.round(2.5) == 3 and Math.round(-2.5) == -2: the WarmUpRateLimiter's cost below the warning line at count 400
    for acquireCount 1 and -1 (only RateLimiterController looks at the sign), seen in latestPassedTime while queueing."""
    assert [ref.jround(x) for x in (2.5, -2.5, -0.5, 0.49999999999999994, -3.5, float("nan"), 1e300, -1e300)] == \
        [3, -2, 0, 0, -3, 0, ref.I64_MAX, ref.I64_MIN]
    ora, mod = _both(400.0, 1, 3, WRL)
    t = 1_700_000_000_000
    for now, prev, acq in [(t, 0, 1), (t + 1000, 400, 1)] + [(t + 1000, 400, 1)] * 5 + [(t + 1000, 400, -1)] * 3:
        before = mod.state()
        assert ora.warm_rl_can_pass(now, prev, acq) == mod.can_pass(now, prev, acq)
        assert ora.state().tolist() == mod.state()
    assert before[0] == 0 < mod.warning_token and mod.state()[2] - before[2] == -2
