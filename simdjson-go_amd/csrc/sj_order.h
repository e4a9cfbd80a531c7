// sj_order.h -- the host-and-device pieces of the orderings (query.hip, sjhip_order_path, sjhip_order_path_strings and sjhip_order_paths): the
// order-preserving key of a number and the chunk key of a string (the sort and its pass plan: sj_sort.h).  Plain C++ under SJ_HD, so the CPU build of a test program can run what the kernels run
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

// The string order compares keys STRORD_CHUNK bytes at a time (query.hip, k_q_order_chunks and k_q_order_place).  The chunk key of the key
// bytes[0 .. len) at byte `at`: the top 56 bits are the bytes [at, at + 7) big-endian, zero padded behind the end of the key; the
// low byte is how many of them are the key's own, min(7, len - at), 0 when at >= len.  The unsigned order of the chunk keys is
// bytes.Compare on the chunks: where the padded bytes tie, the shorter chunk -- a proper prefix, "a" in front of "a" + NUL -- has the
// smaller count.  A count below 7 also says that the key ends inside this chunk; 7 that it may go on.  A descending order sorts
// the complement of the whole chunk key, as the numeric order does with its key.
static constexpr int STRORD_CHUNK = 7;
SJ_HD u64 strord_chunk(const u8 *bytes, u64 len, u64 at) {
    u64 k = 0, count = 0;
    for (int b = 0; b < STRORD_CHUNK; b++) {
        k <<= 8;
        if (at < len && (u64)b < len - at) k |= bytes[at + (u64)b], count++;
    }
    return k << 8 | count;
}
SJ_HD u32 strord_chunk_count(u64 chunk, bool desc) { return (u32)((desc ? ~chunk : chunk) & 0xffu); }
// the rounds that order keys of at most `longest` bytes: the round at byte 7 j sees the end of every key shorter than 7 (j + 1)
SJ_HD u64 strord_max_rounds(u64 longest) { return longest / STRORD_CHUNK + 1; }

// The order by several keys (query.hip, the k_q_order_* kernels; a single-key call is the one-column case) refines classes of tied rows column by column.
// A round of a column sorts its entries by (class, missing, chunk key): the rows without an OK key on the column lie behind the
// others of their class, and tie.  The second sort's key is class << 1 | missing -- classes number at most 2^30, so it is a u32.
// An entry goes on to the column's next round iff it has a key, its new class has company and its chunk was full (a numeric
// column has one round: its chunk is never "full"); whoever still has company when the column ends meets the next column.
static constexpr int ORDER_MAX_KEYS = 8;        // SJHIP_ORDER_MAX_KEYS (query.hip asserts it)
static constexpr int ORDER_KIND_MULTI = -1;     // the kind of the order product after sjhip_order_paths (sj_result.h Order::kind)
SJ_HD u32 mkord_class_key(u32 cls, bool missing) { return cls << 1 | (missing ? 1u : 0u); }
SJ_HD bool mkord_stays(bool missing, bool alone, bool chunk_full) { return !missing && !alone && chunk_full; }

}  // namespace sj
