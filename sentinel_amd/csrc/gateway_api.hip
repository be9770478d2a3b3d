// gateway_api.hip — the front of the gateway path for a batch of HTTP requests: which custom APIs a request's path
// matches (GatewayApiMatcherManager's matchers, SentinelGatewayFilter.pickMatchingApiDefinitions) and the entries the
// filter makes of it (SentinelGatewayFilter.filter: the route entry, then one entry per matching API), written as the
// records sg_gateway_parse_batch and sg_slot_decide_batch take. One request per lane, twice:
//
//   k_gwx<false>  count: every refusal into one error word (ranges, verdict slices), then the request's matches, and
//                 its entries and items into cnt / cnt_items
//   scan          the dictionary's exclusive u64 scan, once over each → the request's first entry and first item (two
//                 u64 sums: a batch cannot overflow them, and the host refuses totals of 2^32 or more)
//   k_gwx<true>   emit: the matches again, and per entry its sg_gateway_req, source index, sg_local_event, context and
//                 one sg_gateway_item per item rule of the entry's resource (the first field of the rule's kind and name)
//
// The match is a merge of four candidate lists, each ascending by definition, so a definition is emitted once and the
// entries come out in definition order without a sort: the exact table's list for the whole path (hash, then byte
// compare), the Ant predicates in the bucket of the path's first segment, the Ant predicates with a wildcard first
// segment, and the definitions behind the request's true verdict ids. Only the last two are walked linearly; work per
// request does not grow with the exact predicates or the literal-first Ant predicates of other buckets. Matching twice
// costs the second pass the same reads (tables and staged path bytes, all read-only) and saves a per-request match
// buffer whose size nothing bounds.
//
// Bounds: a lane reads its path, fields and verdicts only after it has proved their ranges inside bytes[n_bytes],
// fields[n_fields] and verdicts[n_verdicts] (both passes; the host stops before the emit pass at a set error word); a
// step's paths are staged in LDS only when the whole range lies inside bytes[n_bytes]. The tables are the host's
// (gateway_api.h): list ranges inside their arrays, pattern ranges inside the blob, resources checked at load.
#include "engine.h"

namespace sg {

namespace {

constexpr int kGwxLanes = 256;         // requests per block step
constexpr uint32_t kGwxStage = 16384;  // LDS bytes staged per step

static_assert(sizeof(sg_gateway_http_req) == 48 && sizeof(sg_gateway_field) == 16 && sizeof(GwaPred) == 16 &&
                  sizeof(sg_local_event) == 32 && sizeof(sg_slot_ext) == 16,
              "record sizes the loads and stores below assume");

__device__ __forceinline__ GwaPred load_pred(const GwaPred* p) {
    const uint4 w = *reinterpret_cast<const uint4*>(p);
    return GwaPred{w.x, w.y, w.z, w.w};
}

__device__ __forceinline__ sg_gateway_field load_field(const sg_gateway_field* p) {
    const uint4 w = *reinterpret_cast<const uint4*>(p);
    return sg_gateway_field{w.x, w.y, w.z, w.w};
}

__device__ __forceinline__ GwRes gwx_res(const GwxArgs& g, uint32_t resource) {
    return resource < g.n_resources ? g.res[resource] : GwRes{0, 0, 0, 0};
}

// The next Ant candidate of list[i, end) at or above definition `from` that matches the path.
__device__ __forceinline__ uint32_t next_ant(const GwxArgs& g, const GwaPred* list, uint32_t& i, uint32_t end,
                                             uint32_t from, const uint8_t* path, uint32_t len) {
    while (i < end) {
        const GwaPred c = load_pred(list + i++);
        if (c.api >= from && gwa_ant_match(g.patterns + c.pat_off, c.pat_len, path, len)) return c.api;
    }
    return kGwaNone;
}

// The smallest definition at or above `from` behind the request's true API verdicts (ascending ids, API ids first).
__device__ __forceinline__ uint32_t next_verdict(const GwxArgs& g, const sg_gateway_http_req& q, uint32_t from) {
    uint32_t best = kGwaNone;
    for (uint32_t j = 0; j < q.verdict_count; ++j) {
        const uint32_t v = g.verdicts[(uint64_t)q.verdict_begin + j];
        if (v >= g.n_api_vids) break;
        for (uint32_t k = g.vid_begin[v]; k < g.vid_begin[v + 1]; ++k) {
            const uint32_t a = g.vid_apis[k];
            if (a >= from) {
                best = a < best ? a : best;
                break;
            }
        }
    }
    return best;
}

__device__ __forceinline__ bool has_verdict(const GwxArgs& g, const sg_gateway_http_req& q, uint32_t vid) {
    for (uint32_t j = 0; j < q.verdict_count; ++j) {
        const uint32_t v = g.verdicts[(uint64_t)q.verdict_begin + j];
        if (v >= vid) return v == vid;
    }
    return false;
}

// One entry: counted, or written at entry e with its items from item position ip on.
template <bool kEmit>
__device__ __forceinline__ void entry(const GwxArgs& g, const sg_gateway_http_req& q, uint64_t r, uint32_t resource,
                                      int32_t mode, uint32_t& e, uint32_t& ip) {
    const GwRes gr = gwx_res(g, resource);
    if (kEmit) {
        const bool route = mode == 0;
        g.req_out[e] = sg_gateway_req{resource, mode, ip, gr.n_items};
        g.src_out[e] = (uint32_t)r;
        g.ev_out[e] = sg_local_event{q.ts_ms, 0, resource, 1, SG_LOCAL_ENTRY, route ? q.origin : 0};
        g.ext_out[e].context = route ? q.context : g.default_context;
        for (uint32_t k = 0; k < gr.n_items; ++k) {
            const uint32_t ri = gr.rule_begin + k;
            const uint32_t kind = (uint32_t)g.rules[ri].parse_strategy;
            const uint32_t vid = g.item_vid[ri];
            uint4 out = make_uint4(0u, 0u, SG_GW_ITEM_NULL, 0u);
            if (g.fields_set && kind <= SG_GW_PARSE_COOKIE) {
                const uint32_t want = g.item_field[ri];
                for (uint32_t f = 0; f < q.field_count; ++f) {
                    const sg_gateway_field fd = load_field(g.fields + (uint64_t)q.field_begin + f);
                    if (fd.kind == kind && (kind < SG_GW_PARSE_HEADER || fd.name_id == want)) {
                        out = make_uint4(fd.off, fd.len, 0u, 0u);
                        break;
                    }
                }
            }
            if (vid != kGwaNone && has_verdict(g, q, vid)) out.z |= SG_GW_ITEM_REGEX_MATCH;
            *reinterpret_cast<uint4*>(g.items_out + (uint64_t)ip + k) = out;
        }
    }
    ++e;
    ip += gr.n_items;
}

template <bool kEmit>
__global__ void __launch_bounds__(kGwxLanes) k_gwx(GwxArgs g) {
    __shared__ uint32_t stage[kGwxStage / 4];
    uint8_t* sb = reinterpret_cast<uint8_t*>(stage);
    const uint64_t rows = kEmit ? g.n : g.n + 1;  // the count pass clears the slot the scan leaves the totals in
    for (uint64_t i0 = (uint64_t)blockIdx.x * kGwxLanes; i0 < rows; i0 += (uint64_t)gridDim.x * kGwxLanes) {
        const uint64_t i1 = min(i0 + (uint64_t)kGwxLanes, g.n);
        // the step's path bytes, from its first and last request (paths laid out in order make the range tight; any other
        // layout only sends lanes to the in-place path below)
        uint64_t lo = 0, hi = 0, a0 = 0;
        bool staged = false;
        if (i1 > i0) {
            lo = g.req[i0].path_off;
            hi = (uint64_t)g.req[i1 - 1].path_off + g.req[i1 - 1].path_len;
            a0 = lo & ~3ull;
            staged = hi > lo && hi <= g.n_bytes && hi - a0 <= kGwxStage;
        }
        if (staged) {
            const uint32_t nb = (uint32_t)(hi - a0), words = nb / 4;
            const uint32_t* src = reinterpret_cast<const uint32_t*>(g.bytes + a0);
            for (uint32_t w = threadIdx.x; w < words; w += kGwxLanes) stage[w] = src[w];
            if (threadIdx.x < (nb & 3u)) sb[4 * words + threadIdx.x] = g.bytes[a0 + 4 * words + threadIdx.x];
        }
        __syncthreads();
        const uint64_t r = i0 + threadIdx.x;
        if (!kEmit && r == g.n) g.cnt[r] = g.cnt_items[r] = 0;
        if (r < i1) {
            const sg_gateway_http_req q = g.req[r];
            uint32_t err = 0;
            if ((uint64_t)q.path_off + q.path_len > g.n_bytes || (uint64_t)q.field_begin + q.field_count > g.n_fields ||
                (uint64_t)q.verdict_begin + q.verdict_count > g.n_verdicts)
                err |= kGwxErrRange;
            if (!kEmit && err == 0) {
                for (uint32_t f = 0; f < q.field_count; ++f) {
                    const sg_gateway_field fd = load_field(g.fields + (uint64_t)q.field_begin + f);
                    if ((uint64_t)fd.off + fd.len > g.n_bytes) err |= kGwxErrRange;
                }
                uint32_t prev = 0;
                for (uint32_t j = 0; j < q.verdict_count; ++j) {
                    const uint32_t v = g.verdicts[(uint64_t)q.verdict_begin + j];
                    if (v >= g.n_vids || (j > 0 && v <= prev)) err |= kGwxErrVerdict;
                    prev = v;
                }
            }
            uint32_t e = 0, ip = 0;  // entries and items so far: counts, or output positions
            if (kEmit) {  // the host went on only with totals below 2^32
                e = (uint32_t)g.cnt[r];
                ip = (uint32_t)g.cnt_items[r];
            }
            if (err == 0) {
                if (q.route != SG_GW_NO_ROUTE) entry<kEmit>(g, q, r, q.route, 0, e, ip);
                const uint32_t len = q.path_len;
                const bool in_stage = staged && q.path_off >= lo && (uint64_t)q.path_off + len <= hi;
                const uint8_t* path = in_stage ? sb + (q.path_off - a0) : g.bytes + q.path_off;
                uint32_t x_i = 0, x_end = 0, b_i = 0, b_end = 0, w_i = 0;
                if (const GwaSlot* s = gwa_find(g.exact, g.exact_mask, g.patterns, gwa_hash(path, len), path, len)) {
                    x_i = s->begin;
                    x_end = x_i + s->count;
                }
                uint32_t tb = 0, te = 0;
                if (gwa_next(path, len, 0, tb, te))
                    if (const GwaSlot* s = gwa_find(g.bucket, g.bucket_mask, g.patterns, gwa_hash(path + tb, te - tb),
                                                    path + tb, te - tb)) {
                        b_i = s->begin;
                        b_end = b_i + s->count;
                    }
                uint32_t cx = x_i < x_end ? g.exact_list[x_i++] : kGwaNone;
                uint32_t cb = next_ant(g, g.ant, b_i, b_end, 0, path, len);
                uint32_t cw = next_ant(g, g.wild, w_i, g.n_wild, 0, path, len);
                uint32_t cv = next_verdict(g, q, 0);
                for (;;) {
                    const uint32_t a = min(min(cx, cb), min(cw, cv));
                    if (a == kGwaNone) break;
                    entry<kEmit>(g, q, r, g.api_res[a], 1, e, ip);
                    if (cx == a) cx = x_i < x_end ? g.exact_list[x_i++] : kGwaNone;
                    if (cb == a) cb = next_ant(g, g.ant, b_i, b_end, a + 1, path, len);
                    if (cw == a) cw = next_ant(g, g.wild, w_i, g.n_wild, a + 1, path, len);
                    if (cv == a) cv = next_verdict(g, q, a + 1);
                }
            }
            if (!kEmit) {
                g.cnt[r] = err ? 0 : e;
                g.cnt_items[r] = err ? 0 : ip;
                if (err) atomicOr(g.err, err);
            }
        }
        __syncthreads();  // the stage is refilled by the next step
    }
}

unsigned gwx_grid(uint64_t n) {
    const uint64_t b = (n + kGwxLanes - 1) / kGwxLanes;
    return (unsigned)(b < 2048 ? (b ? b : 1) : 2048);
}

}  // namespace

hipError_t launch_gwx_count(const GwxArgs& g, hipStream_t stream) {
    if (((uintptr_t)g.bytes & 3u) != 0) return hipErrorInvalidValue;  // staged loads are 4-byte words
    lds_poison(stream);
    hipLaunchKernelGGL(k_gwx<false>, dim3(gwx_grid(g.n + 1)), dim3(kGwxLanes), 0, stream, g);
    return hipGetLastError();
}

hipError_t launch_gwx_emit(const GwxArgs& g, hipStream_t stream) {
    if (((uintptr_t)g.bytes & 3u) != 0) return hipErrorInvalidValue;
    lds_poison(stream);
    hipLaunchKernelGGL(k_gwx<true>, dim3(gwx_grid(g.n)), dim3(kGwxLanes), 0, stream, g);
    return hipGetLastError();
}

}  // namespace sg
