// gateway.hip — GatewayFlowSlot's request parameter parser (GatewayParamParser.parseParameterFor, sentinel-api-gateway
// -adapter-common/.../param/GatewayParamParser.java:51-84, :156-174) for a batch of requests. The caller's
// RequestItemParser has already pulled the raw strings out of the HTTP request (one item per item rule of the request's
// resource); what is left is per-request, per-rule string work and the exact string → value id mapping:
//
//   k_gw_count   one request per lane: the resource's table, the resource-mode predicate (any item rule of another
//                mode empties the array), the checks that refuse a batch (into one error word), the request's arg and
//                value counts, and for every item of a live request who reads it and as which value (item_map)
//   scan         the dictionary's exclusive u64 scan over args << 32 | values → arg_begin and value_begin
//   k_gw_match   one item per lane: the item bytes of a block step staged in LDS with aligned word loads where they
//                fit (read in place where they do not), gw_match against the rule's pattern, then the dictionary's
//                read-only lookup of the kept string, or the id of "$NM". A second loop writes the "$D" ids.
//   vd_finish    the dictionary's dedupe / rank / commit passes over the misses (pcodec.hip)
//   k_gw_emit    one request per lane: its sg_pslot_arg records and the arg span in sg_slot_ext / sg_pslot_event
//
// Bounds: k_gw_count proves every item range inside items[n_items] and every non-null item's bytes inside
// bytes[n_bytes] before k_gw_match runs (the host stops at a set error word); a step is staged only when its whole
// byte range lies inside bytes[n_bytes], so the staging loads never leave the buffer either.
#include "engine.h"
#include "vdict_dev.h"

namespace sg {

namespace {

constexpr int kGwLanes = 256;         // requests / items per block step
constexpr uint32_t kGwStage = 16384;  // LDS bytes staged per step
constexpr uint64_t kLow32 = 0xFFFFFFFFull;

static_assert(sizeof(sg_gateway_req) == 16 && sizeof(sg_gateway_item) == 16 && sizeof(sg_pslot_arg) == 16,
              "16-byte records: one load or store each");

__device__ __forceinline__ sg_gateway_req load_req(const sg_gateway_req* p) {
    const uint4 w = *reinterpret_cast<const uint4*>(p);
    return sg_gateway_req{w.x, (int32_t)w.y, w.z, w.w};
}

__device__ __forceinline__ sg_gateway_item load_item(const sg_gateway_item* p) {
    const uint4 w = *reinterpret_cast<const uint4*>(p);
    return sg_gateway_item{w.x, w.y, w.z, w.w};
}

__device__ __forceinline__ GwRes res_of(const GwArgs& g, uint32_t resource) {
    return resource < g.n_resources ? g.res[resource] : GwRes{0, 0, 0, 0};
}

__global__ void __launch_bounds__(kGwLanes) k_gw_count(GwArgs g) {
    for (uint64_t r = (uint64_t)blockIdx.x * kGwLanes + threadIdx.x; r <= g.n; r += (uint64_t)gridDim.x * kGwLanes) {
        if (r == g.n) {  // the scan leaves the totals here
            g.cnt[r] = 0;
            break;
        }
        const sg_gateway_req q = load_req(g.req + r);
        const GwRes gr = res_of(g, q.resource);
        uint32_t err = 0;
        if (q.item_count != gr.n_items) err |= kGwErrItemCount;
        if ((uint64_t)q.item_begin + q.item_count > g.n_items) err |= kGwErrRange;
        uint64_t c = 0;
        if (err == 0) {
            const GwItemRule* rules = g.rules + gr.rule_begin;
            bool live = true;  // predSet.size() > 1 || predSet.contains(false) empties the array
            for (uint32_t k = 0; k < gr.n_items; ++k) live &= rules[k].resource_mode == q.resource_mode;
            uint32_t nv = 0;
            for (uint32_t k = 0; k < gr.n_items; ++k) {
                const uint64_t i = (uint64_t)q.item_begin + k;
                const sg_gateway_item it = load_item(g.items + i);
                const bool null = (it.flags & SG_GW_ITEM_NULL) != 0;
                if (!null && (it.len >= (1u << 24) || (uint64_t)it.off + it.len > g.n_bytes)) err |= kGwErrRange;
                const bool val = !null && (uint32_t)rules[k].parse_strategy <= SG_GW_PARSE_COOKIE;  // else parseInternal: null
                if (live) {
                    const uint64_t m = ((r + 1) << 32) | ((uint64_t)nv << 1) | (val ? 1u : 0u);
                    if (atomicExch((unsigned long long*)&g.item_map[i], (unsigned long long)m) != 0ull) err |= kGwErrShared;
                }
                nv += val;
            }
            if (live) c = ((uint64_t)(gr.n_items + gr.has_item_less) << 32) | (uint64_t)(nv + gr.has_item_less);
        }
        g.cnt[r] = c;
        if (err) atomicOr(g.err, err);
    }
}

__global__ void __launch_bounds__(kGwLanes) k_gw_match(GwArgs g) {
    __shared__ uint32_t stage[kGwStage / 4];
    uint8_t* sb = reinterpret_cast<uint8_t*>(stage);
    for (uint64_t i0 = (uint64_t)blockIdx.x * kGwLanes; i0 < g.n_items; i0 += (uint64_t)gridDim.x * kGwLanes) {
        const uint64_t i1 = min(i0 + (uint64_t)kGwLanes, g.n_items);
        // the step's byte range, from its first and last item (items laid out in order make it tight; any other layout,
        // null or unread items with stray offsets included, only sends lanes to the in-place path below)
        const sg_gateway_item first = load_item(g.items + i0), last = load_item(g.items + (i1 - 1));
        const uint64_t lo = first.off, hi = (uint64_t)last.off + last.len;
        const uint64_t a0 = lo & ~3ull;
        const bool staged = hi > lo && hi <= g.n_bytes && hi - a0 <= kGwStage;
        if (staged) {
            const uint32_t nb = (uint32_t)(hi - a0), words = nb / 4;
            const uint32_t* src = reinterpret_cast<const uint32_t*>(g.bytes + a0);
            for (uint32_t w = threadIdx.x; w < words; w += kGwLanes) stage[w] = src[w];
            if (threadIdx.x < (nb & 3u)) sb[4 * words + threadIdx.x] = g.bytes[a0 + 4 * words + threadIdx.x];
        }
        __syncthreads();
        const uint64_t i = i0 + threadIdx.x;
        const uint64_t m = i < i1 ? g.item_map[i] : 0;
        if (m & 1u) {  // a live request reads this item as a value
            const sg_gateway_item it = load_item(g.items + i);
            const uint64_t r = (m >> 32) - 1;
            const sg_gateway_req q = load_req(g.req + r);
            const GwItemRule rule = g.rules[g.res[q.resource].rule_begin + (uint32_t)(i - q.item_begin)];
            const uint64_t j = (g.cnt[r] & kLow32) + ((m & kLow32) >> 1);
            const bool in_stage = staged && it.off >= lo && (uint64_t)it.off + it.len <= hi;
            const uint8_t* p = in_stage ? sb + (it.off - a0) : g.bytes + it.off;
            if (gw_match(rule.match_strategy, p, it.len, g.patterns + rule.pat_off, rule.pat_len,
                         (it.flags & SG_GW_ITEM_REGEX_MATCH) != 0))
                vd_lookup_store(g.vd, j, SG_PARAM_TYPE_STRING, p, it.off, it.len);
            else
                g.vd.ids[j] = g.nm_id;  // SentinelGatewayConstants.GATEWAY_NOT_MATCH_PARAM
        }
        __syncthreads();  // the stage is refilled by the next step
    }
    // GATEWAY_DEFAULT_PARAM: the last value of a live request whose resource has an item-less rule
    for (uint64_t r = (uint64_t)blockIdx.x * kGwLanes + threadIdx.x; r < g.n; r += (uint64_t)gridDim.x * kGwLanes) {
        const uint64_t c0 = g.cnt[r], c1 = g.cnt[r + 1];
        if (((c1 - c0) >> 32) == 0) continue;
        if (g.res[g.req[r].resource].has_item_less) g.vd.ids[(c1 & kLow32) - 1] = g.d_id;
    }
}

__global__ void __launch_bounds__(kGwLanes) k_gw_emit(GwArgs g) {
    for (uint64_t r = (uint64_t)blockIdx.x * kGwLanes + threadIdx.x; r < g.n; r += (uint64_t)gridDim.x * kGwLanes) {
        const uint64_t c0 = g.cnt[r], c1 = g.cnt[r + 1];
        const uint32_t ab = (uint32_t)(c0 >> 32), ac = (uint32_t)((c1 - c0) >> 32);
        if (g.ext) {
            g.ext[r].arg_begin = ab;
            g.ext[r].arg_count = ac;
            g.ext[r].args_null = 0;  // parseParameterFor never returns null
        }
        if (g.pev) {
            g.pev[r].arg_begin = ab;
            g.pev[r].arg_count = ac;
            g.pev[r].args_null = 0;
        }
        if (ac == 0) continue;
        const sg_gateway_req q = load_req(g.req + r);
        const GwRes gr = g.res[q.resource];
        uint32_t v = (uint32_t)(c0 & kLow32);
        uint4* out = reinterpret_cast<uint4*>(g.args + ab);
        for (uint32_t k = 0; k < gr.n_items; ++k) {
            const uint32_t val = (uint32_t)(g.item_map[(uint64_t)q.item_begin + k] & 1u);
            out[k] = make_uint4(v, val, val ? SG_ARG_VALUE : SG_ARG_NULL, 0u);
            v += val;
        }
        if (gr.has_item_less) out[gr.n_items] = make_uint4(v, 1u, SG_ARG_VALUE, 0u);
    }
}

unsigned gw_grid(uint64_t n) {
    const uint64_t b = (n + kGwLanes - 1) / kGwLanes;
    return (unsigned)(b < 2048 ? (b ? b : 1) : 2048);
}

}  // namespace

hipError_t launch_gw_count(const GwArgs& g, hipStream_t stream) {
    hipLaunchKernelGGL(k_gw_count, dim3(gw_grid(g.n + 1)), dim3(kGwLanes), 0, stream, g);
    return hipGetLastError();
}

hipError_t launch_gw_match(const GwArgs& g, hipStream_t stream) {
    if (((uintptr_t)g.bytes & 3u) != 0) return hipErrorInvalidValue;  // staged loads are 4-byte words
    lds_poison(stream);
    hipLaunchKernelGGL(k_gw_match, dim3(gw_grid(g.n_items > g.n ? g.n_items : g.n)), dim3(kGwLanes), 0, stream, g);
    return hipGetLastError();
}

hipError_t launch_gw_emit(const GwArgs& g, hipStream_t stream) {
    hipLaunchKernelGGL(k_gw_emit, dim3(gw_grid(g.n)), dim3(kGwLanes), 0, stream, g);
    return hipGetLastError();
}

}  // namespace sg
