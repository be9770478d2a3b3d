// table_sweep.h — when an entry of an exact value table is idle: the predicates of sg_param_sweep / sg_cparam_sweep.
// Plain functions for host and device, no HIP runtime in here: the sweep kernels (grow.hip) call them per slot, and
// tests/cpp/test_table_sweep_host.cpp checks them on the CPU against a restatement of the walkers' steps.
//
// An entry is idle at `now` when, for every t >= now, the walker's step gives the same answer and leaves the same state
// whether the entry is present or absent. Removing exactly those entries changes no decision.
//
//   token bucket (behaviour != RATE_LIMITER, param_default_step, ParamFlowChecker.java:147-201)
//       with both counters present, a positive tokenCount and now - time > duration, the step takes the refill
//       branch; once (now - time) * tc / dur + tokens > maxCount it sets tokens = maxCount - acquire and time = t and
//       passes — what the first sight of a value does. passTime only grows with t, so the comparison stays true. The
//       arithmetic is Java's long: a product or sum that would wrap there is never called idle (the wrapped value could
//       land on the other side of the comparison), so every intermediate is checked for overflow here; past now the
//       equivalence reaches as far as the reference's own product does, t - time < 2^63 / tc ms. A slot
//       with one counter missing (flags 1 or 2, which no walker leaves behind) is kept.
//   throttle (behaviour 2, param_throttle_step, :214-253)
//       never idle. A fresh value passes any acquireCount at once; a recorded time puts expected = time + cost, and a
//       large enough acquireCount makes cost exceed any distance t - time, so the request queues or blocks where a
//       fresh value would pass.
//   claimed, never counted (a value word with flags 0)
//       not in the reference's maps: dropped, as a resize drops it, and counted apart.
//   cluster param ring (ClusterParamMetric's LeapArray)
//       idle iff every written bucket has now - start > intervalMs, the strict > of LeapArray.isWindowDeprecated and
//       of the walker's window (cp_window counts start >= windowStart(t) - (S - 1) * wl, and windowStart(t) > t - wl).
//       Such a ring sums to 0 and currentWindow resets whichever bucket it lands on: a never-written ring.
//   thread count (ParameterMetric.threadCountMap)
//       idle iff the count is 0 — the remove of ParameterMetric.decreaseThreadCount (:184-239), whatever the time.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SG_SWEEP_FN __host__ __device__ inline
#else
#define SG_SWEEP_FN inline
#endif

namespace sg {

enum SweepVerdict : uint32_t {
    kSweepKeep = 0,   // carried over
    kSweepIdle = 1,   // given back: no later request can tell it from absence
    kSweepClaim = 2,  // claimed and never counted: given back, counted apart
};

// tc: param_token_count(rule, value), hot items included; dur_ms: duration_sec * 1000.
SG_SWEEP_FN bool sweep_token_idle(uint32_t flags, int64_t time, int64_t tokens, int64_t tc, int64_t burst,
                                  int64_t dur_ms, int64_t now) {
    if (flags != 3u || tc <= 0 || dur_ms <= 0) return false;
    int64_t maxc, pass_time, prod, sum;
    if (__builtin_add_overflow(tc, burst, &maxc)) return false;
    if (__builtin_sub_overflow(now, time, &pass_time)) return false;
    if (!(pass_time > dur_ms)) return false;
    if (__builtin_mul_overflow(pass_time, tc, &prod)) return false;  // wraps in Java: never idle
    if (__builtin_add_overflow(prod / dur_ms, tokens, &sum)) return false;
    return sum > maxc;
}

// behavior: PRule::behavior (2 = throttle). The verdict on one PSlot's counters; the caller has seen a value word.
SG_SWEEP_FN SweepVerdict sweep_pslot(uint32_t flags, int64_t time, int64_t tokens, int32_t behavior, int64_t tc,
                                     int64_t burst, int64_t dur_ms, int64_t now) {
    if (!flags) return kSweepClaim;
    if (behavior == 2) return kSweepKeep;
    return sweep_token_idle(flags, time, tokens, tc, burst, dur_ms, now) ? kSweepIdle : kSweepKeep;
}

// One bucket of a ring: never written, or deprecated at now.
SG_SWEEP_FN bool sweep_bucket_gone(int64_t start, int64_t interval_ms, int64_t now) {
    if (start == INT64_MIN) return true;
    int64_t age;
    if (__builtin_sub_overflow(now, start, &age)) return false;
    return age > interval_ms;
}

// ring[0 .. S): anything with an int64_t `start` (CPBucket on the device). interval_ms = sampleCount * windowLengthMs.
template <class Bucket>
SG_SWEEP_FN SweepVerdict sweep_ring(const Bucket* ring, int S, int64_t interval_ms, int64_t now) {
    bool written = false, live = false;
    for (int j = 0; j < S; ++j) {
        const int64_t start = ring[j].start;
        written = written || start != INT64_MIN;
        live = live || !sweep_bucket_gone(start, interval_ms, now);
    }
    return !written ? kSweepClaim : live ? kSweepKeep : kSweepIdle;
}

SG_SWEEP_FN bool sweep_thread_idle(int64_t count) { return count <= 0; }

}  // namespace sg
