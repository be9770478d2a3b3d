"""A plain-Python restatement of the reference's two warm-up controllers, written from the Java text alone:

    sentinel-core/.../slots/block/flow/controller/WarmUpController.java:83-175
        construct (:83-106), canPass (:113-138), syncToken (:140-159), coolDownTokens (:161-175)
    sentinel-core/.../slots/block/flow/controller/WarmUpRateLimiterController.java:43-87
        canPass

It is the guard of oracle/sentinel_oracle.c's controller code (tests/test_shaping_kat.py), which the device code is
nearly a transcription of: a shared misreading of the Java there would pass every parity test. Nothing here is taken
from either. Java's arithmetic is spelled out on Python ints (explicit 32- and 64-bit two's-complement wrap) and
Python floats (IEEE doubles, one rounding per operation, as Java's strictfp-by-default doubles):

    (int) / (long) of a double   JLS §5.1.3: NaN -> 0, saturating, else toward zero
    int / int                    JLS §15.17.2: truncates toward zero
    double / 0.0                 JLS §15.17.2: +-Infinity, or NaN for 0.0 / 0.0 and NaN operands
    Math.round(double)           floor(a + 1/2) exactly (ties toward +Infinity), NaN -> 0, saturating
    Math.nextUp(double)          NaN -> NaN, +Infinity -> +Infinity
    long -> double               round to nearest even (Python's float(int) does the same)

The time is a parameter (TimeUtil.currentTimeMillis()), the node's passQps() / previousPassQps() are parameters
(doubles, as Node returns them), Thread.sleep is the returned wait, and a single caller means every compareAndSet
succeeds. Every controller counts the branches it takes into `visits` (a collections.Counter).
"""
import collections
import math

I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1

VISITS = collections.Counter()
BRANCHES = ("below", "equal", "above", "above_refill", "capped", "clamped", "nan_qps", "qps_below_1")


def i32(x):
    """An int operation's result, wrapped to 32 bits."""
    return ((x - I32_MIN) & 0xFFFFFFFF) + I32_MIN


def i64(x):
    """A long operation's result, wrapped to 64 bits."""
    return ((x - I64_MIN) & 0xFFFFFFFFFFFFFFFF) + I64_MIN


def _narrow(x, lo, hi):
    if x != x:
        return 0
    if x >= hi:  # the int bound is exact as a float: at or above hi's float (2^31 - 1 exactly, 2^63 for long) saturates
        return hi
    if x <= lo:
        return lo
    return int(x)  # toward zero


def d2i(x):
    """(int) x."""
    return _narrow(x, I32_MIN, I32_MAX)


def d2l(x):
    """(long) x."""
    return _narrow(x, I64_MIN, I64_MAX)


def idiv(a, b):
    """int / int, b != 0."""
    q = abs(a) // abs(b)
    return i32(q if (a < 0) == (b < 0) else -q)


def ddiv(a, b):
    """double / double."""
    if b == 0.0:
        if a != a or a == 0.0:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def jround(a):
    """Math.round(double)."""
    if a != a:
        return 0
    if abs(a) >= 4503599627370496.0:  # 2^52: no fraction bits left
        return d2l(a)
    f = math.floor(a)
    return f + 1 if a - f >= 0.5 else f  # a - floor(a) is exact below 2^52


def next_up(a):
    """Math.nextUp(double)."""
    return math.nextafter(a, math.inf)


class WarmUpController:
    def __init__(self, count, warm_up_period_in_sec, cold_factor=3, visits=None):
        self.visits = VISITS if visits is None else visits
        # construct (:83-106)
        if cold_factor <= 1:                                                     # :85-87
            raise ValueError("Cold factor should be larger than 1")
        count = float(count)
        self.count = count                                                       # :89
        self.cold_factor = cold_factor                                           # :91
        # :95 warningToken = (int)(warmUpPeriodInSec * count) / (coldFactor - 1): int * double, cast, int / int
        self.warning_token = idiv(d2i(float(warm_up_period_in_sec) * count), i32(cold_factor - 1))
        # :99 maxToken = warningToken + (int)(2 * warmUpPeriodInSec * count / (1.0 + coldFactor)): the first product is
        # int * int, then * double, / double; int + int
        two_w = i32(2 * warm_up_period_in_sec)
        self.max_token = i32(self.warning_token + d2i(ddiv(float(two_w) * count, 1.0 + float(cold_factor))))
        # :104 slope = (coldFactor - 1.0) / count / (maxToken - warningToken): the difference is an int
        self.slope = ddiv(ddiv(float(cold_factor) - 1.0, count), float(i32(self.max_token - self.warning_token)))
        self.stored_tokens = 0                                                   # :72 AtomicLong(0)
        self.last_filled_time = 0                                                # :73 AtomicLong(0)

    def _warning_qps(self, above_token):
        """Math.nextUp(1.0 / (aboveToken * slope + 1.0 / count)) (:127, WarmUpRateLimiterController.java:56):
        long * double, double + double."""
        q = next_up(ddiv(1.0, float(above_token) * self.slope + ddiv(1.0, self.count)))
        if q != q:
            self.visits["nan_qps"] += 1
        elif q < 1.0:
            self.visits["qps_below_1"] += 1
        return q

    def can_pass(self, now, pass_qps, previous_pass_qps, acquire_count=1):
        """canPass (:113-138)."""
        pass_qps = d2l(float(pass_qps))                                          # :115
        previous_qps = d2l(float(previous_pass_qps))                             # :117
        self.sync_token(now, previous_qps)                                       # :118
        rest_token = self.stored_tokens                                          # :122
        total = float(i64(pass_qps + acquire_count))                             # long + int, then compared as a double
        if rest_token >= self.warning_token:                                     # :123
            above_token = i64(rest_token - self.warning_token)                   # :124
            return total <= self._warning_qps(above_token)                       # :127-130
        return total <= self.count                                               # :132-134

    def sync_token(self, now, pass_qps):
        """syncToken (:140-159)."""
        current_time = now - now % 1000                                          # :141-142 (the time is not negative)
        if current_time <= self.last_filled_time:                                # :143-146
            return
        new_value = self.cool_down_tokens(current_time, pass_qps)                # :149
        self.stored_tokens = new_value                                           # :151
        current_value = i64(self.stored_tokens - pass_qps)                       # :152 addAndGet(0 - passQps)
        self.stored_tokens = current_value
        if current_value < 0:                                                    # :153-155
            self.visits["clamped"] += 1
            self.stored_tokens = 0
        self.last_filled_time = current_time                                     # :156

    def _refill(self, old_value, current_time):
        """(long)(oldValue + (currentTime - lastFilledTime.get()) * count / 1000) (:168, :171): long * double, / int as
        a double, long + double."""
        dt = i64(current_time - self.last_filled_time)
        return d2l(float(old_value) + float(dt) * self.count / 1000.0)

    def cool_down_tokens(self, current_time, pass_qps):
        """coolDownTokens (:161-175)."""
        old_value = self.stored_tokens                                           # :162
        new_value = old_value                                                    # :163
        if old_value < self.warning_token:                                       # :167
            self.visits["below"] += 1
            new_value = self._refill(old_value, current_time)                    # :168
        elif old_value > self.warning_token:                                     # :169
            self.visits["above"] += 1
            if pass_qps < idiv(d2i(self.count), self.cold_factor):               # :170 (int)count / coldFactor
                self.visits["above_refill"] += 1
                new_value = self._refill(old_value, current_time)                # :171
        else:
            self.visits["equal"] += 1
        if new_value > self.max_token:
            self.visits["capped"] += 1
        return min(new_value, self.max_token)                                    # :174

    def state(self):
        return [self.stored_tokens, self.last_filled_time, -1]


class WarmUpRateLimiterController(WarmUpController):
    def __init__(self, count, warm_up_period_sec, time_out_ms, cold_factor=3, visits=None):
        super().__init__(count, warm_up_period_sec, cold_factor, visits)          # :33
        self.timeout_in_ms = time_out_ms                                         # :34
        self.latest_passed_time = -1                                             # :30 AtomicLong(-1)

    def can_pass(self, now, previous_pass_qps, acquire_count=1):
        """canPass (WarmUpRateLimiterController.java:43-87): (passed, the Thread.sleep)."""
        previous_qps = d2l(float(previous_pass_qps))                             # :44
        self.sync_token(now, previous_qps)                                       # :45
        current_time = now                                                       # :47
        rest_token = self.stored_tokens                                          # :49
        if rest_token >= self.warning_token:                                     # :52
            above_token = i64(rest_token - self.warning_token)                   # :53
            warming_qps = self._warning_qps(above_token)                         # :56
            cost_time = jround(ddiv(1.0 * float(acquire_count), warming_qps) * 1000.0)   # :57
        else:
            cost_time = jround(ddiv(1.0 * float(acquire_count), self.count) * 1000.0)    # :59
        expected_time = i64(cost_time + self.latest_passed_time)                 # :61
        if expected_time <= current_time:                                        # :63
            self.latest_passed_time = current_time                               # :64
            return True, 0
        wait_time = i64(i64(cost_time + self.latest_passed_time) - current_time)  # :67
        if wait_time > self.timeout_in_ms:                                       # :68-69
            return False, 0
        old_time = self.latest_passed_time = i64(self.latest_passed_time + cost_time)  # :71 addAndGet: the new value
        wait_time = i64(old_time - current_time)                                 # :73 (the same instant)
        if wait_time > self.timeout_in_ms:                                       # :74-77
            self.latest_passed_time = i64(self.latest_passed_time - cost_time)
            return False, 0
        return True, max(wait_time, 0)                                           # :78-81

    def state(self):
        return [self.stored_tokens, self.last_filled_time, self.latest_passed_time]
