// gossip_protocol_amd/csrc/reach_row.hpp -- what the overlay-reach kernels (reach_kernels.hip,
// reach_multi_kernels.hip) share: the alive rule, the bitmap test and the edge rule of both
// tables.  Device-only.
#pragma once
#include "scale_row.hpp"

namespace gsp {

__device__ __forceinline__ bool reach_alive_at(const int32_t *start_tick, const int32_t *fail_tick,
                                               int32_t tick, int32_t r) {
    return (start_tick ? start_tick[r] : 0) <= tick && tick <= fail_tick[r];
}

__device__ __forceinline__ bool reach_bit(const uint64_t *map, uint32_t x) {
    return (reinterpret_cast<const uint32_t *>(map)[x >> 5] >> (x & 31u)) & 1u;
}

// ---- full view ----
// present & fresh of the two entries of a word: 1 in bit 0 / bit 16 (the census's arithmetic)
__device__ __forceinline__ uint32_t reach_fresh(uint32_t w, uint32_t t5x2, uint32_t lim) {
    const uint32_t pe = pk_min(w, 0x00010001u);                  // present: e != 0
    const uint32_t age = pk_sub(t5x2, w) & 0x001F001Fu;          // (T - ts) mod 32
    return pk_min(pk_subc(lim, age), pe);                        // age < age_limit
}

// the four words' flags as one bit per entry, entry q of the lane vector in bit q
__device__ __forceinline__ uint32_t reach_pack(const uint32_t (&f)[4]) {
    uint32_t m = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) m |= ((f[i] | (f[i] >> 15)) & 3u) << (2 * i);
    return m;
}

// ---- partial view ----
// the id of a slot and whether it is an edge's: an id >= n is dropped before it becomes an address
__device__ __forceinline__ bool reach_entry_at(uint64_t e, int32_t n, int32_t tick, int32_t age_limit,
                                               uint32_t &id) {
    id = uint32_t(e >> 32);
    return id < uint32_t(n) && ((uint32_t(tick) - uint32_t(e)) & 31u) < uint32_t(age_limit);
}

}  // namespace gsp
