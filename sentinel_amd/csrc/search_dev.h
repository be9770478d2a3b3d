// search_dev.h — device helpers shared by every kernel file: the 64-lane wave primitives (sum, min, scans, lane
// masks), wave-wide and per-lane searches over sorted data, the window average's division.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sg {

__device__ __forceinline__ int lane_id() { return (int)__lane_id(); }

// the lanes below f as a ballot mask
__device__ __forceinline__ uint64_t below(int f) { return f >= 64 ? ~0ull : ((1ull << f) - 1ull); }

__device__ __forceinline__ int64_t wave_sum(int64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor((long long)v, o, 64);
    return v;
}

__device__ __forceinline__ int64_t wave_min(int64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, (int64_t)__shfl_xor((long long)v, o, 64));
    return v;
}

__device__ __forceinline__ int64_t wave_incl_scan(int64_t v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int64_t y = __shfl_up((long long)v, (unsigned)o, 64);
        if (lane >= o) v += y;
    }
    return v;
}

__device__ __forceinline__ int64_t wave_excl_scan(int64_t v, int lane) { return wave_incl_scan(v, lane) - v; }

// The largest i in [lo, hi) with key(i) <= x, for keys ascending and key(lo) <= x (a table whose entry lo is unused
// or known to qualify is never read there).
template <class I, class X, class Key>
__device__ __forceinline__ I last_le(I lo, I hi, X x, Key key) {
    while (hi - lo > 1) {
        const I mid = (lo + hi) >> 1;
        if (key(mid) <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}

// First q in [lo, hi) with pred(q) (pred monotone false → true), hi if none: 64 evenly spaced probes per step, so a
// million-record range takes 4 dependent loads.
template <class Pred>
__device__ __forceinline__ uint64_t search64(uint64_t lo, uint64_t hi, Pred pred, int lane) {
    while (hi - lo > 64) {
        const uint64_t step = (hi - lo + 63) / 64;
        const uint64_t q = lo + (uint64_t)lane * step;
        const uint64_t m = __ballot(q >= hi || pred(q));
        if (m == 0) {
            lo = lo + 63 * step + 1;
            continue;
        }
        const int f = __builtin_ctzll(m);
        if (f == 0) return lo;
        const uint64_t nhi = lo + (uint64_t)f * step;
        lo = lo + (uint64_t)(f - 1) * step + 1;
        hi = nhi < hi ? nhi : hi;
    }
    const uint64_t q = lo + (uint64_t)lane;
    const uint64_t m = __ballot(q < hi && pred(q));
    return m ? lo + (uint64_t)__builtin_ctzll(m) : hi;
}

// As search64 for an answer expected near lo (a segment's end seen from inside it, a window period's end): lane l
// probes lo + 2^l - 1, which brackets the answer between two probes (the first few share lo's cache line), then
// search64 inside the bracket. search64 over [lo, hi) alone spreads its first rounds over the whole range — 64 far
// cache lines per round when hi is the end of the batch.
template <class Pred>
__device__ __forceinline__ uint64_t gallop_search(uint64_t lo, uint64_t hi, Pred pred, int lane) {
    if (lo >= hi) return hi;
    const uint64_t span = hi - lo;
    const uint64_t off = lane < 63 ? (1ull << lane) - 1ull : ~0ull;
    const bool in = off < span;
    const uint64_t m = __ballot(!in || pred(lo + off));  // lane 63 is never in: m != 0
    const int f = __builtin_ctzll(m);
    if (f == 0) return lo;
    const uint64_t b0 = lo + (1ull << (f - 1));            // probe f - 1 (at b0 - 1) was false
    const uint64_t b1 = lo + ((1ull << f) - 1ull);          // probe f: true, or past hi
    return search64(b0, b1 < hi ? b1 : hi, pred, lane);
}

// A batch's period table: bnd[q] is the first request index of period q (entry 0 unused); the period of request idx.
__device__ __forceinline__ uint32_t period_of(const uint32_t* bnd, uint32_t np, uint32_t idx) {
    return last_le(0u, np, idx, [&](uint32_t q) { return bnd[q]; });
}

// One lane's own search: is v in the sorted a[0 .. n)? (AuthoritySlot's origin ids above 64: a handful per resource.)
__device__ __forceinline__ bool sorted_has(const int32_t* a, uint32_t n, int32_t v) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && a[lo] == v;
}

// sum / intervalInSecond (LeapArray averages: ClusterMetric.getAvg, StatisticNode.passQps, …) as Java computes it.
// For a power-of-two interval (1 s, 2 s, 0.5 s, …) the quotient is the product with the exact reciprocal, built from
// the exponent bits; the fp64 division sequence (~13 instructions a record on the walkers' hot path) runs only
// for other intervals. (A test for isec == 1.0 alone is folded away by the compiler: x / 1.0 == x.)
__device__ __forceinline__ double avg_div(double x, double isec) {
    const uint64_t b = (uint64_t)__double_as_longlong(isec);
    const uint64_t e = (b >> 52) & 0x7FF;
    if ((b & 0x800FFFFFFFFFFFFFull) == 0 && e - 1 < 0x7FD)
        return x * __longlong_as_double((long long)((0x7FEull - e) << 52));
    return x / isec;
}

// Streaming stores for the prep kernels' outputs (default results, packed records: written once, read by a later
// kernel): non-temporal, so a batch's front half does not fill L2 with lines the walkers beside it would have used.
template <class T>
__device__ __forceinline__ void st_stream(T* p, T v) {
    __builtin_nontemporal_store(v, p);
}

}  // namespace sg
