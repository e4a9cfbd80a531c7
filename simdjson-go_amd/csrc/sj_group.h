// sj_group.h -- the host-and-device pieces of the grouping (query.hip, sjhip_group_path and sjhip_group_paths): the hash of a key
// column's entry, the fold of a tuple's hash from them, and the equality of two keys.  Plain C++ under SJ_HD, so the CPU build of a
// test program can run what the kernels run.
//
// The hash only places a key in the open-addressing table; the result of the grouping does not depend on it (groups are numbered
// by first occurrence, equality is decided by the bytes).  Strings are hashed 8 bytes at a time -- a multiply-xorshift round per
// word, the tail bytes gathered into one last word, the length mixed in -- and an int64 key is one finalising mix.
#pragma once
#include "sj_chunk.h"  // SJ_HD, u8 / u32 / u64

namespace sj {

static constexpr u32 GROUP_NONE = 0xffffffffu;  // SJHIP_GROUP_NONE, and the empty slot of the table

SJ_HD u64 group_mix(u64 h) {  // (the finaliser of MurmurHash3: every input bit reaches every output bit)
    h ^= h >> 33;
    h *= 0xff51afd7ed558ccdull;
    h ^= h >> 33;
    h *= 0xc4ceb9fe1a85ec53ull;
    h ^= h >> 33;
    return h;
}
SJ_HD u64 group_hash_int(u64 x) { return group_mix(x ^ 0x9e3779b97f4a7c15ull); }
SJ_HD u64 group_hash_bytes(const u8 *s, u64 len) {
    u64 h = 0x9e3779b97f4a7c15ull ^ (len * 0xff51afd7ed558ccdull);
    u64 k = 0;
    for (; k + 8 <= len; k += 8) {
        u64 w;
        __builtin_memcpy(&w, s + k, 8);  // (no alignment is promised: a key lies anywhere in Strings.B or the message)
        h = (h ^ group_mix(w)) * 0x9fb21c651e98df25ull;
        h ^= h >> 29;
    }
    u64 w = 0;
    for (u32 j = 0; k < len; k++, j += 8) w |= (u64)s[k] << j;
    return group_mix(h ^ w);
}
SJ_HD bool group_bytes_equal(const u8 *a, const u8 *b, u64 len) {
    u64 k = 0;
    for (; k + 8 <= len; k += 8) {
        u64 x, y;
        __builtin_memcpy(&x, a + k, 8);
        __builtin_memcpy(&y, b + k, 8);
        if (x != y) return false;
    }
    for (; k < len; k++)
        if (a[k] != b[k]) return false;
    return true;
}
// The hash of a row's tuple of key columns (k_q_group_keys) begins as column 0's hash above -- of the column's bytes or of its 8-byte
// value; GROUP_NO_KEY_HASH where the row has no key on the column -- and every later column's is folded in.  So a tuple of one
// column hashes as that column (the home slots tests/group_table.py constructs hold for sjhip_group_path and for sjhip_group_paths
// alike).  The fold depends on the order of the columns (the running hash is multiplied before the column's is added), and for a
// fixed non-empty prefix it is a bijection of the last column's hash: an addition, then the invertible group_mix --
// tests/group_multi_table.py solves an INT last column for a chosen tuple hash that way.
static constexpr u64 GROUP_NO_KEY_HASH = 0x6a09e667f3bcc909ull;
SJ_HD u64 group_tuple_fold(u64 acc, u64 h) { return group_mix(acc * 0x9fb21c651e98df25ull + h); }

// the power-of-two capacity of the table of n rows: at least twice the rows, so that every probe sequence meets an empty slot
SJ_HD u64 group_table_capacity(u64 n) {
    u64 cap = 64;
    while (cap < 2 * n) cap <<= 1;
    return cap;
}

}  // namespace sj
