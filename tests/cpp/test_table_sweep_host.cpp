// TEST INFRASTRUCTURE: the idle predicates of the table sweep (sentinel_amd/csrc/table_sweep.h) on the CPU, against a
// restatement of the walkers' steps: an entry the predicate calls idle must be indistinguishable from absence for
// every later request, and entries just short of idle must be kept and must be distinguishable. Its own main, no GPU,
// no HIP; built with the address and undefined-behaviour sanitizers by table_sweep_host.mk.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <random>

#include "../../sentinel_amd/csrc/table_sweep.h"

namespace {

int failures = 0;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            ++failures;                                                    \
            fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #cond); \
        }                                                                  \
    } while (0)

// Java long arithmetic wraps: the restatement computes in uint64_t where the device code relies on -fwrapv.
int64_t wmul(int64_t a, int64_t b) { return (int64_t)((uint64_t)a * (uint64_t)b); }
int64_t wadd(int64_t a, int64_t b) { return (int64_t)((uint64_t)a + (uint64_t)b); }
int64_t wsub(int64_t a, int64_t b) { return (int64_t)((uint64_t)a - (uint64_t)b); }

struct PState {
    int64_t time, tokens;
    uint32_t flags;
    bool operator==(const PState& o) const { return time == o.time && tokens == o.tokens && flags == o.flags; }
};

// ParamFlowChecker.passDefaultLocalCheck (ParamFlowChecker.java:147-201), as pslot_dev.h's param_default_step
bool default_step(PState& s, int64_t tc, int64_t maxc, int64_t dur, int64_t t, int64_t acq) {
    if (!(s.flags & 1u)) {
        s.flags |= 1u;
        s.time = t;
        if (!(s.flags & 2u)) {
            s.flags |= 2u;
            s.tokens = wsub(maxc, acq);
        }
        return true;
    }
    const int64_t pass_time = wsub(t, s.time);
    if (pass_time > dur) {
        if (!(s.flags & 2u)) {
            s.flags |= 2u;
            s.tokens = wsub(maxc, acq);
            s.time = t;
            return true;
        }
        const int64_t rest = s.tokens;
        const int64_t to_add = wmul(pass_time, tc) / dur;
        const int64_t nq = wadd(to_add, rest) > maxc ? wsub(maxc, acq) : wsub(wadd(rest, to_add), acq);
        if (nq < 0) return false;
        s.tokens = nq;
        s.time = t;
        return true;
    }
    if ((s.flags & 2u) && s.tokens - acq >= 0) {
        s.tokens -= acq;
        return true;
    }
    return false;
}

// passThrottleLocalCheck (:214-253), as param_throttle_step
bool throttle_step(PState& s, int64_t cost, int32_t max_queue, int64_t t) {
    if (!(s.flags & 1u)) {
        s.flags |= 1u;
        s.time = t;
        return true;
    }
    const int64_t expected = s.time + cost;
    if (expected <= t || expected - t < max_queue) {
        s.time = t;
        if (expected - t > 0) s.time = expected;
        return true;
    }
    return false;
}

// The walker's step on one value: passSingleValueCheck rejects tokenCount 0 and acquire > maxCount before it reads
// the maps (ParamFlowChecker.java:137-146; k_pprep and ps_single do the same), then passDefaultLocalCheck.
bool walker_step(PState& s, int64_t tc, int64_t maxc, int64_t dur, int64_t t, int64_t acq) {
    if (tc == 0 || acq > maxc) return false;
    return default_step(s, tc, maxc, dur, t, acq);
}

// true when a request (t, acq) cannot tell `present` from an absent entry: the same pass bit, and the same state
// after — or neither side touched (an early rejection), which leaves the question as it was
bool same_as_absent(const PState& present, int64_t tc, int64_t maxc, int64_t dur, int64_t t, int64_t acq) {
    const PState absent{0, 0, 0};
    PState a = present, b = absent;
    const bool pa = walker_step(a, tc, maxc, dur, t, acq);
    const bool pb = walker_step(b, tc, maxc, dur, t, acq);
    return pa == pb && (a == b || (a == present && b == absent));
}

bool invisible_from(const PState& s, int64_t tc, int64_t burst, int64_t dur, int64_t now) {
    const int64_t maxc = tc + burst;
    const int64_t ts[4] = {now, now + 1, now + dur, now + 10 * dur};
    for (int64_t t : ts)
        for (int64_t acq = -1; acq <= maxc + 1; ++acq)
            if (!same_as_absent(s, tc, maxc, dur, t, acq)) return false;
    return true;
}

void test_token_buckets() {
    std::mt19937_64 rng(20260921);
    auto draw = [&](int64_t lo, int64_t hi) { return lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1)); };
    int idle = 0, kept = 0, kept_visible = 0;
    for (int it = 0; it < 20000; ++it) {
        const int64_t tc = draw(1, 50), burst = draw(0, 20), dur = draw(1, 3) * 1000;
        const int64_t maxc = tc + burst;
        PState s{draw(0, 100000), draw(0, maxc), 3u};
        const int64_t now = s.time + draw(0, 4 * dur);
        const bool is_idle = sg::sweep_token_idle(s.flags, s.time, s.tokens, tc, burst, dur, now);
        CHECK(sg::sweep_pslot(s.flags, s.time, s.tokens, 0, tc, burst, dur, now) == (is_idle ? sg::kSweepIdle : sg::kSweepKeep));
        if (is_idle) {
            ++idle;
            CHECK(invisible_from(s, tc, burst, dur, now));
        } else {
            ++kept;
            kept_visible += !invisible_from(s, tc, burst, dur, now);
        }
    }
    CHECK(idle > 1000);
    CHECK(kept > 1000);
    CHECK(kept_visible > 1000);  // the predicate is not vacuous: kept entries that a request can tell from absence

    // one millisecond short of the duration: kept, and visible (the no-refill branch pays from the 0 tokens left)
    {
        const int64_t tc = 5, burst = 2, dur = 1000;
        PState s{10000, 0, 3u};
        CHECK(!sg::sweep_token_idle(3u, s.time, s.tokens, tc, burst, dur, s.time + dur));
        CHECK(!same_as_absent(s, tc, tc + burst, dur, s.time + dur, 1));
        // the tokens here refill past the maximum one millisecond later only if the refill is large enough
        PState full{10000, tc + burst, 3u};
        CHECK(!sg::sweep_token_idle(3u, full.time, full.tokens, tc, burst, dur, full.time + dur));
        CHECK(sg::sweep_token_idle(3u, full.time, full.tokens, tc, burst, dur, full.time + dur + 1));
        CHECK(invisible_from(full, tc, burst, dur, full.time + dur + 1));
    }
    // short of the refill: the predicate is the step's own strict toAdd + tokens > maxCount
    {
        const int64_t tc = 5, burst = 2, dur = 1000;  // maxCount 7
        const int64_t now = 10000 + 1200;             // toAdd = 1200 * 5 / 1000 = 6
        PState s2{10000, 2, 3u};                      // 6 + 2 > 7: idle
        CHECK(sg::sweep_token_idle(3u, s2.time, s2.tokens, tc, burst, dur, now));
        CHECK(invisible_from(s2, tc, burst, dur, now));
        PState s1{10000, 1, 3u};                      // 6 + 1 == 7: one token short of the predicate, kept
        CHECK(!sg::sweep_token_idle(3u, s1.time, s1.tokens, tc, burst, dur, now));
        PState s0{10000, 0, 3u};                      // 6 + 0 < 7: one token short of a full bucket, kept and visible:
        CHECK(!sg::sweep_token_idle(3u, s0.time, s0.tokens, tc, burst, dur, now));
        CHECK(!same_as_absent(s0, tc, tc + burst, dur, now, 1));  // the step leaves 5 tokens, a fresh value 6
    }
    // flags, tokenCount 0, half-present counters
    CHECK(!sg::sweep_token_idle(1u, 0, 7, 5, 2, 1000, 100000));
    CHECK(!sg::sweep_token_idle(2u, 0, 7, 5, 2, 1000, 100000));
    CHECK(!sg::sweep_token_idle(3u, 0, 7, 0, 2, 1000, 100000));
    CHECK(sg::sweep_pslot(0u, 0, 0, 0, 5, 2, 1000, 100000) == sg::kSweepClaim);
    CHECK(sg::sweep_pslot(0u, 0, 0, 2, 5, 2, 1000, 100000) == sg::kSweepClaim);
}

void test_overflow_guard() {
    // (now - time) * tc wraps in Java: the wrapped product can be negative, the step then keeps rest + toAdd — an
    // entry a fresh value differs from. Never idle, whatever the wrapped comparison would say.
    const int64_t dur = 1000, burst = 0;
    const int64_t tc = INT64_MAX / 4, time = 0, now = 100000;  // 100000 * 2^61 wraps
    CHECK(!sg::sweep_token_idle(3u, time, 1, tc, burst, dur, now));
    // the largest product that fits is still decided by the comparison
    const int64_t tc2 = INT64_MAX / 100000;
    CHECK(sg::sweep_token_idle(3u, time, tc2, tc2, burst, dur, now));
    PState s{time, tc2, 3u};
    CHECK(same_as_absent(s, tc2, tc2 + burst, dur, now, 1));
    // tokenCount + burst, now - time and toAdd + tokens that would wrap
    CHECK(!sg::sweep_token_idle(3u, 0, 1, INT64_MAX, 1, dur, now));
    CHECK(!sg::sweep_token_idle(3u, INT64_MIN + 5, 1, 5, 0, dur, now));
    CHECK(!sg::sweep_token_idle(3u, 0, INT64_MAX, 5, 0, dur, now));
}

void test_throttle() {
    // never idle: a recorded time blocks a large enough acquireCount at any distance, a fresh value passes it
    CHECK(sg::sweep_pslot(1u, 1000, 0, 2, 5, 0, 1000, INT64_MAX / 2) == sg::kSweepKeep);
    PState present{1000, 0, 1u}, absent{0, 0, 0};
    const int64_t t = 1000 + 1000000000LL;   // far later
    const int64_t cost = 2 * 1000000000LL;   // round(1000 * acq * dur / tc) of a large acquireCount
    CHECK(!throttle_step(present, cost, 0, t));
    CHECK(throttle_step(absent, cost, 0, t));
}

struct Bucket {
    int64_t start, count;
};

// ClusterParamMetric.getSum at t over a ring, as cparam_dev.h's cp_window (the valid buckets of the window at t)
int64_t ring_sum(const Bucket* ring, int S, int64_t wl, int64_t t) {
    const int64_t P = t / wl, ws = P * wl, lo = ws - (int64_t)(S - 1) * wl;
    int64_t sum = 0;
    for (int j = 0; j < S; ++j)
        if (ring[j].start != INT64_MIN && ring[j].start >= lo && ring[j].start <= ws) sum += ring[j].count;
    return sum;
}

// addValue at t: currentWindow resets a stale bucket, then adds
void ring_add(Bucket* ring, int S, int64_t wl, int64_t t, int64_t n) {
    const int64_t P = t / wl, ws = P * wl;
    Bucket& b = ring[P % S];
    if (b.start != ws) {
        b.start = ws;
        b.count = 0;
    }
    b.count += n;
}

void test_rings() {
    for (int S : {2, 10}) {
        const int64_t wl = 1000 / S * 3, interval = S * wl;
        // a never-written ring is a claim; one written bucket decides at the boundary
        Bucket ring[10], fresh[10];
        for (int j = 0; j < 10; ++j) ring[j] = fresh[j] = Bucket{INT64_MIN, 0};
        CHECK(sg::sweep_ring(ring, S, interval, 1000000) == sg::kSweepClaim);
        const int64_t start = 50 * wl;
        ring[50 % S] = Bucket{start, 7};
        CHECK(sg::sweep_ring(ring, S, interval, start + interval) == sg::kSweepKeep);      // now - start == interval
        CHECK(sg::sweep_ring(ring, S, interval, start + interval + 1) == sg::kSweepIdle);  // interval + 1
        CHECK(!sg::sweep_bucket_gone(start, interval, start + interval));
        CHECK(sg::sweep_bucket_gone(start, interval, start + interval + 1));
        // idle: every later sum and every later add agree with a never-written ring
        const int64_t now = start + interval + 1;
        for (int64_t t : {now, now + 1, now + wl, now + interval, now + 10 * interval}) {
            CHECK(ring_sum(ring, S, wl, t) == 0);
            Bucket a[10], b[10];
            for (int j = 0; j < 10; ++j) {
                a[j] = ring[j];
                b[j] = fresh[j];
            }
            ring_add(a, S, wl, t, 3);
            ring_add(b, S, wl, t, 3);
            for (int64_t u : {t, t + wl, t + interval})
                CHECK(ring_sum(a, S, wl, u) == ring_sum(b, S, wl, u));
        }
        // a second, live bucket keeps the whole ring
        ring[51 % S] = Bucket{start + wl, 2};
        CHECK(sg::sweep_ring(ring, S, interval, now) == sg::kSweepKeep);
        CHECK(sg::sweep_ring(ring, S, interval, start + wl + interval + 1) == sg::kSweepIdle);
        // kept rings are not vacuous: within the window a written bucket is visible
        CHECK(ring_sum(ring, S, wl, start + wl) != 0);
    }
}

void test_thread_counts() {
    CHECK(sg::sweep_thread_idle(0));
    CHECK(!sg::sweep_thread_idle(1));
    CHECK(!sg::sweep_thread_idle(INT64_MAX));
}

}  // namespace

int main() {
    test_token_buckets();
    test_overflow_guard();
    test_throttle();
    test_rings();
    test_thread_counts();
    if (failures) {
        fprintf(stderr, "%d failures\n", failures);
        return 1;
    }
    printf("table sweep host ok\n");
    return 0;
}
