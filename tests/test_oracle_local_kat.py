"""Known-answer tests of the local slot-chain oracle (StatisticSlot → FlowSlot/DefaultController →
DegradeSlot), restating the reference's own tests on the replay model:

  ExceptionCircuitBreakerTest.testRecordErrorOrSuccess   sentinel-core/src/test/.../degrade/circuitbreaker/ExceptionCircuitBreakerTest.java:50-83
  ResponseTimeCircuitBreakerTest.testMaxSlowRatioThreshold                                  …/ResponseTimeCircuitBreakerTest.java:30-53
  CircuitBreakingIntegrationTest.{testSlowRequestMode, testExceptionRatioMode, testMultipleHalfOpenedBreakers}
                                                         sentinel-core/src/test/.../degrade/CircuitBreakingIntegrationTest.java:55-230
  DefaultControllerTest.{testCanPassForQps, testCanPassForThreadCount}   …/flow/controller/DefaultControllerTest.java:33-57

The Java tests drive a mocked TimeUtil (AbstractTimeBasedTest: sleep() advances the clock; an entry
that passes sleeps inside the try, then exits). `Clock` below is the same harness over explicit event
times. Random sleeps (ThreadLocalRandom ranges) are drawn from a seeded generator over several seeds:
the assertions of the reference hold for every value in those ranges.
"""
import numpy as np
import pytest

from oracle.binding import LocalChain, degrade_rule, local_rule
from sentinel_amd import abi

OPEN, CLOSED, HALF_OPEN = 1, 0, 2


class Clock:
    """AbstractTimeBasedTest over the oracle (sentinel-core/src/test/.../test/AbstractTimeBasedTest.java)."""

    def __init__(self, chain, t0=0, res=0):
        self.c, self.t, self.res = chain, t0, res

    def sleep(self, ms):
        self.t += ms

    def entry_and_sleep_for(self, ms):
        st, _ = self.c.entry(self.t, self.res)
        if st in (abi.LOCAL_BLOCK_FLOW, abi.LOCAL_BLOCK_DEGRADE):
            return False
        create = self.t
        self.sleep(ms)
        self.c.exit(self.t, create, self.res)
        return True

    def entry_with_error_if_present(self, error, sleep_ms):
        st, _ = self.c.entry(self.t, self.res)
        if st in (abi.LOCAL_BLOCK_FLOW, abi.LOCAL_BLOCK_DEGRADE):
            return False
        create = self.t
        self.sleep(sleep_ms)
        self.c.exit(self.t, create, self.res, error=error)
        return True


def chain_with(*breakers, flow=None):
    c = LocalChain()
    fc, fg = flow if flow else (0.0, abi.FLOW_GRADE_NONE)
    c.load_rules(np.array([local_rule(fc, fg, breakers)]))
    return c


@pytest.mark.parametrize("seed", range(6))
def test_exception_breaker_record_error_or_success(seed):
    rnd = np.random.default_rng(seed)
    r = lambda: int(rnd.integers(5, 10))  # ThreadLocalRandom.nextInt(5, 10)
    retry_ms = 10 * 1000
    c = chain_with(degrade_rule(abi.DEGRADE_EXCEPTION_RATIO, 0.2, retry_ms // 1000, min_request_amount=1,
                                stat_interval_ms=20 * 1000))
    k = Clock(c, t0=0)
    assert k.entry_and_sleep_for(10)
    assert k.entry_with_error_if_present(True, r())  # -> open
    assert not k.entry_with_error_if_present(True, r())
    assert not k.entry_and_sleep_for(100)
    k.sleep(retry_ms // 2)
    assert not k.entry_and_sleep_for(100)
    k.sleep(retry_ms // 2)
    assert k.entry_with_error_if_present(True, r())  # -> half -> open
    assert not k.entry_and_sleep_for(100)
    assert not k.entry_and_sleep_for(100)
    k.sleep(retry_ms)
    assert k.entry_and_sleep_for(100)  # -> half -> closed
    for _ in range(6):
        assert k.entry_and_sleep_for(100)
    assert k.entry_with_error_if_present(True, r())
    assert k.entry_and_sleep_for(100)


def test_rt_breaker_max_slow_ratio_threshold():
    c = chain_with(degrade_rule(abi.DEGRADE_RT, 10, 5, min_request_amount=3, stat_interval_ms=5000,
                                slow_ratio_threshold=1.0))
    k = Clock(c, t0=0)
    assert k.entry_and_sleep_for(20)
    assert k.entry_and_sleep_for(20)
    assert k.entry_and_sleep_for(20)
    # should be blocked: 3/3 requests' rt is bigger than max rt
    assert not k.entry_and_sleep_for(20)
    k.sleep(1000)
    assert not k.entry_and_sleep_for(20)
    k.sleep(4000)
    assert k.entry_and_sleep_for(20)


T0_SEC = 1_700_000_123_000  # setCurrentMillis(System.currentTimeMillis() / 1000 * 1000)


@pytest.mark.parametrize("seed", range(6))
def test_integration_slow_request_mode(seed):
    rnd = np.random.default_rng(100 + seed)
    ri = lambda lo, hi: int(rnd.integers(lo, hi))
    retry, max_rt, stat, min_req = 5, 50, 20000, 10
    c = chain_with(degrade_rule(abi.DEGRADE_RT, max_rt, retry, min_request_amount=min_req, stat_interval_ms=stat,
                                slow_ratio_threshold=0.8))
    k = Clock(c, t0=T0_SEC)
    for i in range(min_req):
        assert k.entry_and_sleep_for(max_rt + (ri(10, 20) if i < 7 else ri(-20, -10)))
    # slow ratio 70 % so far
    for _ in range(6):
        assert k.entry_and_sleep_for(max_rt + ri(10, 20))
    assert c.breaker(0, 0)[0] == OPEN
    assert not k.entry_and_sleep_for(1)
    k.sleep(1000)
    assert not k.entry_and_sleep_for(1)
    k.sleep(retry * 1000)
    assert k.entry_and_sleep_for(max_rt + ri(10, 20))  # HALF_OPEN → OPEN
    assert c.breaker(0, 0)[0] == OPEN
    k.sleep((retry + 1) * 1000)
    assert k.entry_and_sleep_for(max_rt - ri(10, 20))  # HALF_OPEN → CLOSED
    assert c.breaker(0, 0)[0] == CLOSED
    assert k.entry_and_sleep_for(max_rt + ri(10, 20))


@pytest.mark.parametrize("seed", range(6))
def test_integration_exception_ratio_mode(seed):
    rnd = np.random.default_rng(200 + seed)
    r = lambda: int(rnd.integers(5, 10))
    retry, min_req = 5, 10
    c = chain_with(degrade_rule(abi.DEGRADE_EXCEPTION_RATIO, 0.5, retry, min_request_amount=min_req,
                                stat_interval_ms=25000))
    k = Clock(c, t0=T0_SEC)
    for i in range(min_req - 1):
        assert k.entry_with_error_if_present(i < 6, r())
    assert k.entry_with_error_if_present(True, r())  # 7/10 → OPEN
    assert c.breaker(0, 0)[0] == OPEN
    assert not k.entry_with_error_if_present(False, r())
    k.sleep(2000)
    assert not k.entry_with_error_if_present(False, r())
    k.sleep(retry * 1000)
    assert k.entry_with_error_if_present(True, r())  # HALF_OPEN → OPEN
    assert c.breaker(0, 0)[0] == OPEN
    k.sleep((retry + 1) * 1000)
    assert k.entry_with_error_if_present(False, r())  # HALF_OPEN → CLOSED
    assert c.breaker(0, 0)[0] == CLOSED
    assert k.entry_with_error_if_present(True, r())


def _verify_state(c, target):
    """CircuitBreakingIntegrationTest.verifyState: OPEN +1, HALF_OPEN -1, CLOSED -2."""
    s = 0
    for i in range(2):
        st = c.breaker(0, i)[0]
        s += 1 if st == OPEN else (-1 if st == HALF_OPEN else -2)
    assert s == target


def test_integration_multiple_half_opened_breakers():
    retry, max_rt, stat = 2, 50, 20000
    c = chain_with(
        degrade_rule(abi.DEGRADE_RT, max_rt, retry, min_request_amount=1, stat_interval_ms=stat,
                     slow_ratio_threshold=0.8),
        degrade_rule(abi.DEGRADE_RT, max_rt, retry * 2, min_request_amount=1, stat_interval_ms=stat,
                     slow_ratio_threshold=0.8))
    k = Clock(c, t0=T0_SEC)
    assert k.entry_and_sleep_for(100)
    assert c.breaker(0, 0)[0] == OPEN and c.breaker(0, 1)[0] == OPEN
    k.sleep(3000)
    for _ in range(10):
        assert not k.entry_and_sleep_for(100)
    # one stays OPEN, the other went OPEN → HALF_OPEN → OPEN (whenTerminate revert)
    _verify_state(c, 2)
    k.sleep(3000)
    for _ in range(10):
        assert k.entry_and_sleep_for(1)
    _verify_state(c, -4)


def test_half_open_revert_keeps_next_retry():
    """AbstractCircuitBreaker.fromOpenToHalfOpen's whenTerminate hook reverts to OPEN without moving
    nextRetryTimestamp (AbstractCircuitBreaker.java:101-120): the next entry probes again at once."""
    c = chain_with(
        degrade_rule(abi.DEGRADE_RT, 50, 2, min_request_amount=1, stat_interval_ms=20000),
        degrade_rule(abi.DEGRADE_RT, 50, 4, min_request_amount=1, stat_interval_ms=20000))
    k = Clock(c, t0=T0_SEC)
    assert k.entry_and_sleep_for(100)
    nr0 = c.breaker(0, 0)[1]
    k.sleep(3000)
    assert not k.entry_and_sleep_for(1)
    assert c.breaker(0, 0) == (OPEN, nr0)


def test_default_controller_qps():
    """DefaultControllerTest.testCanPassForQps: passQps threshold-1 → pass, threshold → block."""
    thr = 10
    c = chain_with(flow=(thr, abi.FLOW_GRADE_QPS))
    t = T0_SEC + 100
    for _ in range(thr - 1):  # passQps = 9 (interval 1 s)
        assert c.entry(t)[0] == abi.LOCAL_PASS
    assert c.second_sum(0, t, 0) == thr - 1
    assert c.entry(t)[0] == abi.LOCAL_PASS   # 9 + 1 <= 10
    assert c.entry(t)[0] == abi.LOCAL_BLOCK_FLOW  # 10 + 1 > 10


def test_default_controller_thread():
    """DefaultControllerTest.testCanPassForThreadCount: curThreadNum 7 → pass, 8 → block."""
    thr = 8
    c = chain_with(flow=(thr, abi.FLOW_GRADE_THREAD))
    t = T0_SEC
    for _ in range(thr - 1):
        assert c.entry(t)[0] == abi.LOCAL_PASS
    assert c.threads(0) == thr - 1
    assert c.entry(t)[0] == abi.LOCAL_PASS
    assert c.entry(t)[0] == abi.LOCAL_BLOCK_FLOW
    c.exit(t + 5, t)  # one thread leaves
    assert c.threads(0) == thr - 1
    assert c.entry(t + 5)[0] == abi.LOCAL_PASS


def test_flow_partial_qps_grade():
    """FlowPartialIntegrationTest.testQPSGrade: count 1 → first passes, second blocked within the second."""
    c = chain_with(flow=(1, abi.FLOW_GRADE_QPS))
    t = T0_SEC + 10
    assert c.entry(t)[0] == abi.LOCAL_PASS
    assert c.entry(t + 1)[0] == abi.LOCAL_BLOCK_FLOW
    assert c.minute_sum(0, t + 1, 1) == 1  # increaseBlockQps


def test_prioritized_occupy_next_window():
    """DefaultController prioritized branch → StatisticNode.tryOccupyNext (StatisticNode.java:288-320):
    a prioritized entry over the threshold borrows from the next 500 ms bucket and passes with a wait;
    the borrowed pass shows up when that bucket becomes current (OccupiableBucketLeapArray.newEmptyBucket)."""
    c = chain_with(flow=(2, abi.FLOW_GRADE_QPS))
    t1 = T0_SEC + 100  # first half-window [T0, T0+500)
    assert c.entry(t1)[0] == abi.LOCAL_PASS
    assert c.entry(t1)[0] == abi.LOCAL_PASS
    t = T0_SEC + 600
    assert c.entry(t)[0] == abi.LOCAL_BLOCK_FLOW
    # the window [T0, T0+500) (2 passes) leaves the interval in 1000 - 600 = 400 ms < occupyTimeout
    st, wait = c.entry(t, prio=True)
    assert (st, wait) == (abi.LOCAL_PASS_WAIT, 400)
    assert c.waiting(0, t) == 1
    assert c.threads(0) == 3
    assert c.minute_sum(0, t, abi.LOCAL_PASS_WAIT + 2) == 1  # OCCUPIED_PASS (ordinal 5)
    # second prioritized entry: 2 + borrow 1 + 1 - 2 = 2 <= 2 → also waits 400 ms
    assert c.entry(t, prio=True) == (abi.LOCAL_PASS_WAIT, 400)
    # third: borrow 2 >= maxCount 2 → occupyTimeout → blocked
    assert c.entry(t, prio=True)[0] == abi.LOCAL_BLOCK_FLOW
    # a prioritized entry without a droppable window: t in the first half → nothing to borrow
    c2 = chain_with(flow=(1, abi.FLOW_GRADE_QPS))
    assert c2.entry(T0_SEC + 600)[0] == abi.LOCAL_PASS
    assert c2.entry(T0_SEC + 700, prio=True)[0] == abi.LOCAL_BLOCK_FLOW
    # at the next bucket the borrowed passes are counted in the current window
    assert c.second_sum(0, T0_SEC + 1000, 0) == 2
    assert c.entry(T0_SEC + 1000)[0] == abi.LOCAL_BLOCK_FLOW


def test_no_rule_resource_passes_and_counts():
    c = chain_with()
    t = T0_SEC
    for i in range(100):
        assert c.entry(t + i)[0] == abi.LOCAL_PASS
    assert c.threads(0) == 100
    assert c.second_sum(0, t + 99, 0) == 100
    for i in range(100):
        c.exit(t + 200 + i, t + i, error=(i % 10 == 0))
    assert c.threads(0) == 0
    assert c.minute_sum(0, t + 300, 2) == 10  # exceptions
    assert c.minute_sum(0, t + 300, 3) == 100  # success
    assert c.minute_sum(0, t + 300, 4) == 100 * 200  # rt sum


# ---- circuit breaker edges the oracle alone answers for (tests/test_breaker_edges_premise.py), by hand

@pytest.mark.parametrize("tw,ms", [(2_147_484, -2147483296), (4_294_968, 704)])
def test_recovery_timeout_wraps_as_an_int(tw, ms):
    """`protected final int recoveryTimeoutMs` (AbstractCircuitBreaker.java:36) = rule.getTimeWindow() * 1000 (:54) in
    int arithmetic: 2 147 484 s wraps to -2 147 483 296 ms (nextRetryTimestamp lies in the past: the next entry is
    the probe), 4 294 968 s to 704 ms. updateNextRetryTimestamp (:89-91) adds it to the long clock."""
    assert (tw * 1000 + (1 << 31)) % (1 << 32) - (1 << 31) == ms
    c = chain_with(degrade_rule(abi.DEGRADE_EXCEPTION_COUNT, 0, tw, min_request_amount=1, stat_interval_ms=1000))
    t = T0_SEC + 17
    assert c.entry(t)[0] == abi.LOCAL_PASS
    c.exit(t + 5, t, error=True)  # 1 > 0: open
    assert c.breaker(0, 0) == (OPEN, t + 5 + ms)
    if ms < 0:
        assert c.entry(t + 5)[0] == abi.LOCAL_PASS and c.breaker(0, 0)[0] == HALF_OPEN
    else:
        assert c.entry(t + 5 + ms - 1)[0] == abi.LOCAL_BLOCK_DEGRADE and c.breaker(0, 0)[0] == OPEN
        assert c.entry(t + 5 + ms)[0] == abi.LOCAL_PASS and c.breaker(0, 0)[0] == HALF_OPEN
    # the probe comes back in error: fromHalfOpenToOpen (:132-139) adds the same wrapped timeout
    t2 = t + 5 + max(ms, 0)
    c.exit(t2 + 9, t2, error=True)
    assert c.breaker(0, 0) == (OPEN, t2 + 9 + ms)


@pytest.mark.parametrize("count,max_rt", [(0.5, 1), (0.49999999999999994, 0), (10.5, 11), (1e30, (1 << 63) - 1)])
def test_max_allowed_rt_is_math_round_of_the_count(count, max_rt):
    """maxAllowedRt = Math.round(rule.getCount()) (ResponseTimeCircuitBreaker.java:52): ties go up (0.5 -> 1, 10.5 ->
    11), the largest double below 0.5 gives 0 (floor(x + 0.5) in double arithmetic would give 1), 1e30 saturates at
    Long.MAX_VALUE. `rt > maxAllowedRt` (:76) counts a slow request. Slow ratio 0.0: the first slow exit opens."""
    c = chain_with(degrade_rule(abi.DEGRADE_RT, count, 1, min_request_amount=1, stat_interval_ms=1 << 30,
                                slow_ratio_threshold=0.0))
    t = T0_SEC + 3
    at = min(max_rt, 1 << 40)
    assert c.entry(t)[0] == abi.LOCAL_PASS
    c.exit(t + at, t)  # rt == maxAllowedRt: not slow
    assert c.breaker(0, 0)[0] == CLOSED and c.breaker_stat(0, 0)[1:] == (0, 1)
    assert c.entry(t + at)[0] == abi.LOCAL_PASS
    if max_rt == (1 << 63) - 1:
        c.exit(t + at + (1 << 41), t + at)
        assert c.breaker(0, 0)[0] == CLOSED and c.breaker_stat(0, 0)[1] == 0
        return
    c.exit(t + at + max_rt + 1, t + at)  # rt == maxAllowedRt + 1: slow, 1 / 2 > 0.0
    assert c.breaker(0, 0)[0] == OPEN and c.breaker_stat(0, 0)[1:] == (1, 2)


def _rt_exits(c, t, rts):
    for i, rt in enumerate(rts):
        assert c.entry(t + i)[0] == abi.LOCAL_PASS
    for i, rt in enumerate(rts):
        c.exit(t + i + rt, t + i)
        yield c.breaker(0, 0)[0]


def test_slow_ratio_equality_opens_only_at_1():
    """handleStateChangeWhenThresholdExceeded (ResponseTimeCircuitBreaker.java:101-118): `currentRatio >
    maxSlowRequestRatio` opens, and so does equality, but only when the threshold is SLOW_REQUEST_RATIO_MAX_VALUE
    (Double.compare(...) == 0 twice, :114-115). At 0.5 a ratio of exactly 0.5 stays CLOSED."""
    rule = lambda thr: degrade_rule(abi.DEGRADE_RT, 10, 1, min_request_amount=2, stat_interval_ms=10_000,  # noqa: E731
                                    slow_ratio_threshold=thr)
    t = T0_SEC + 11
    # 1.0: one slow exit is below the amount; two of two: 1.0 == 1.0 opens; a fast one among them never does
    assert list(_rt_exits(chain_with(rule(1.0)), t, [11, 12])) == [CLOSED, OPEN]
    assert list(_rt_exits(chain_with(rule(1.0)), t, [11, 10, 12, 13])) == [CLOSED] * 4
    # 0.5: 1 / 2 == 0.5 stays CLOSED, 2 / 4 too, 3 / 5 opens
    assert list(_rt_exits(chain_with(rule(0.5)), t, [11, 10, 10, 12, 13])) == [CLOSED] * 4 + [OPEN]


@pytest.mark.parametrize("count,n_closed", [(3, 3), (2.5, 2), (0, 0)])
def test_exception_count_is_compared_with_greater_than(count, n_closed):
    """`curCount > threshold` with a double threshold (ExceptionCircuitBreaker.java:105-112): 3 errors against 3 stay
    CLOSED and the fourth opens; against 2.5 two stay CLOSED and the third opens."""
    c = chain_with(degrade_rule(abi.DEGRADE_EXCEPTION_COUNT, count, 1, min_request_amount=1, stat_interval_ms=10_000))
    t = T0_SEC + 29
    for i in range(n_closed + 1):
        assert c.entry(t + i)[0] == abi.LOCAL_PASS
    for i in range(n_closed + 1):
        assert c.breaker(0, 0)[0] == CLOSED
        c.exit(t + 20 + i, t + i, error=True)
    assert c.breaker(0, 0)[0] == OPEN and c.breaker_stat(0, 0)[1] == n_closed + 1
