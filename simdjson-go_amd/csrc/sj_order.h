// sj_order.h -- the host-and-device piece of the ordering (query.hip, sjhip_order_path): the order-preserving key of a number (the
// sort and its pass plan: sj_sort.h).  Plain C++ under SJ_HD, so the CPU build of a test program can run what the kernels run
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

}  // namespace sj
