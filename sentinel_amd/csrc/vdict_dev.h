// vdict_dev.h — the value dictionary's device-side key functions: canonical payload, hash, byte compare and the
// read-only lookup of one batch value. One copy for every kernel file that names values through the dictionary
// (pcodec.hip: the param-flow wire codec and the dictionary's own passes; gateway.hip: the gateway param parser).
#pragma once
#include "engine.h"

namespace sg {

// The canonical payload of a value of at most 8 bytes, byte k in bits [8k, 8k + 8): as on the wire, except BOOLEAN
// 00 / 01 (readBoolean: non-zero is true) and one NaN per float width (Double.equals / Float.equals compare
// doubleToLongBits / floatToIntBits, which collapse every NaN).
__device__ __forceinline__ uint64_t canonical_inline(uint32_t type, const uint8_t* p, uint32_t len) {
    uint64_t v = 0;
    for (uint32_t k = 0; k < len; ++k) v |= (uint64_t)p[k] << (8 * k);
    if (type == SG_PARAM_TYPE_BOOLEAN) return v != 0;
    if (type == SG_PARAM_TYPE_DOUBLE) {
        const uint64_t bits = __builtin_bswap64(v);
        if ((bits & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull) return __builtin_bswap64(0x7FF8000000000000ull);
    } else if (type == SG_PARAM_TYPE_FLOAT) {
        const uint32_t bits = __builtin_bswap32((uint32_t)v);
        if ((bits & 0x7FFFFFFFu) > 0x7F800000u) return (uint64_t)__builtin_bswap32(0x7FC00000u);
    }
    return v;
}

// hash of (type, length, canonical payload): 8-byte little-endian chunks, the last zero-padded; a payload of at most
// 8 bytes is the one chunk `inl` (sentinel_amd/param_wire.py value_hash is the mirror)
__device__ __forceinline__ uint64_t value_hash(uint32_t tl, uint64_t inl, const uint8_t* p) {
    uint64_t h = mix64((uint64_t)tl);
    const uint32_t len = tl >> 8;
    if (len <= 8) return mix64(h ^ inl);
    for (uint32_t b = 0; b < len; b += 8) {
        uint64_t w = 0;
        const uint32_t e = min(8u, len - b);
        for (uint32_t k = 0; k < e; ++k) w |= (uint64_t)p[b + k] << (8 * k);
        h = mix64(h ^ w);
    }
    return h;
}

__device__ __forceinline__ bool bytes_eq(const uint8_t* a, const uint8_t* b, uint32_t len) {
    for (uint32_t k = 0; k < len; ++k)
        if (a[k] != b[k]) return false;
    return true;
}

// Value j of the batch: p = its payload bytes (LDS or HBM), off = where they lie in v.src. Writes its descriptor and
// hash and looks it up in the main table (read-only): v.ids[j] = its id, or 0 for a miss.
__device__ __forceinline__ void vd_lookup_store(const VDictArgs& v, uint64_t j, uint32_t type, const uint8_t* p,
                                                uint32_t off, uint32_t len) {
    VDesc d;
    d.off = off;
    d.tl = (len << 8) | type;
    d.inl = len <= 8 ? canonical_inline(type, p, len) : 0;
    const uint64_t h = value_hash(d.tl, d.inl, p);
    v.desc[j] = d;
    v.hash[j] = h;
    uint64_t id = 0;
    for (uint64_t s = h & v.tab_mask;; s = (s + 1) & v.tab_mask) {  // at most half of the slots are ever taken
        const uint64_t t = v.tab[s];
        if (t == 0) break;
        if ((t >> 32) != (h >> 32)) continue;
        const VEntry e = v.entries[t & 0xFFFFFFFFu];
        if (e.hash != h || e.len != len || e.type != type) continue;
        if (len <= 8 ? e.data == d.inl : bytes_eq(v.arena + e.data, p, len)) {
            id = t & 0xFFFFFFFFu;
            break;
        }
    }
    v.ids[j] = id;
    const uint64_t mm = __ballot(id == 0);  // one add per wave
    if (id == 0 && (int)(threadIdx.x & 63) == __ffsll((unsigned long long)mm) - 1)
        atomicAdd(v.n_miss, (unsigned long long)__popcll(mm));
}

}  // namespace sg
