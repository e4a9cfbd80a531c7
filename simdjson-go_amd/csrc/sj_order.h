// sj_order.h -- the host-and-device pieces of the ordering (query.hip, sjhip_order_path): the order-preserving key of a number, the
// geometry of the sort and its pass plan.  Plain C++ under SJ_HD, so the CPU build of a test program can run what the kernels run
// (host_selftest.cpp, tests/test_order_result_state.py).
//
// The key of a FLOAT, INT or UINT value is a uint64 whose unsigned order is the order of the kind (the min / max of the aggregates
// compare the same keys): UINT as it is; INT with the sign bit flipped; FLOAT with all bits of a negative value flipped and the sign
// bit of the others, the total order of the non-NaN doubles with -0.0 below +0.0.  A descending order sorts the complement of the
// key ascending, so that a stable sort leaves equal keys in row order in both directions.
#pragma once
#include "sj_chunk.h"  // SJ_HD, u8 / u32 / u64

namespace sj {

static constexpr int ORDER_KIND_FLOAT = 0, ORDER_KIND_INT = 1, ORDER_KIND_UINT = 2;  // SJHIP_COL_FLOAT / INT / UINT (query.hip asserts it)
static constexpr u64 AGG_SIGN = 0x8000000000000000ull;
SJ_HD u64 agg_key(u64 x, int kind) {
    if (kind == ORDER_KIND_UINT) return x;
    if (kind == ORDER_KIND_INT) return x ^ AGG_SIGN;
    return (x >> 63) ? ~x : x ^ AGG_SIGN;
}
SJ_HD u64 agg_unkey(u64 k, int kind) {
    if (kind == ORDER_KIND_UINT) return k;
    if (kind == ORDER_KIND_INT) return k ^ AGG_SIGN;
    return (k >> 63) ? k ^ AGG_SIGN : ~k;
}

// the radix sort of the (key, row) pairs: ORDER_RADIX_BITS per pass, tiles of ORDER_SORT_TILE rows (ORDER_SORT_THREADS threads,
// ORDER_SORT_ROUNDS rows each, taken in rounds so that the order inside a tile is the row order), at most ORDER_PASSES passes
static constexpr int ORDER_RADIX_BITS = 8, ORDER_RADIX = 1 << ORDER_RADIX_BITS, ORDER_PASSES = 64 / ORDER_RADIX_BITS;
static constexpr int ORDER_SORT_THREADS = 256, ORDER_SORT_ROUNDS = 4, ORDER_SORT_TILE = ORDER_SORT_THREADS * ORDER_SORT_ROUNDS;

// The pass plan: bit p is set iff the sort takes the pass over digit p (bits 8p .. 8p + 7 of the key).  and_ / or_: the AND and the
// OR of all keys that are sorted; a bit that is equal in both is equal in every key, and a digit of such bits orders nothing.
// Equal keys (and a single key) take no pass.
SJ_HD u32 order_pass_mask(u64 and_, u64 or_) {
    const u64 varying = and_ ^ or_;
    u32 mask = 0;
    for (int p = 0; p < ORDER_PASSES; p++)
        if ((varying >> (ORDER_RADIX_BITS * p)) & (u64)(ORDER_RADIX - 1)) mask |= 1u << p;
    return mask;
}
SJ_HD u32 order_pass_count(u32 mask) {
    u32 c = 0;
    for (; mask; mask &= mask - 1) c++;
    return c;
}

}  // namespace sj
