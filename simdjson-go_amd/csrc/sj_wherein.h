// sj_wherein.h -- the host-and-device pieces of the set predicate (query.hip, sjhip_where_path_in): the caller's values as a set on the
// device, the open-addressing table over them, and the probe a row's key makes.  Plain C++ under SJ_HD, so the CPU build of a test
// program (host_selftest.cpp) runs what the kernels run: the table is reached through a policy -- device-scope atomics in
// k_q_in_build, plain loads and stores in the replay.
//
// The table is the grouping's (sj_group.h: hash, byte equality, capacity) with the SET's values in the place of the rows: slot ->
// the index of a value, GROUP_NONE where it is empty, linear probing from hash & mask.  Equal values end in one slot that holds the
// smallest of their indices, so which values the table holds, and under which index, is decided by the set alone; where a value
// lies inside its chain depends on the order of the inserts, which no probe can tell.
#pragma once
#include "sj_bounds.h"
#include "sj_group.h"

namespace sj {

static constexpr int IN_KIND_STRING = 4;  // SJHIP_COL_STRING; every other kind of a set is an 8-byte value
static constexpr u32 IN_MAX_STRING = 1024;  // the longest value EQ_STRING takes: a longer key of a row equals nothing

struct InSet {
    int kind;
    u32 n, mask;           // values (duplicates included); capacity - 1 = group_table_capacity(n) - 1
    Arr<const u64> vals;   // [n] the values' bits; STRING: [n + 1] the offsets of the values in `bytes`
    Arr<const u8> bytes;   // STRING: the values end to end
    Arr<u64> hash;         // [n] written by the build, read by the probes
    Arr<u32> table;        // [mask + 1]
};

SJ_HD u64 in_len(const InSet &s, u32 j) { return s.vals[j + 1] - s.vals[j]; }
SJ_HD u64 in_value_hash(const InSet &s, u32 j) {
    if (s.kind != IN_KIND_STRING) return group_hash_int(s.vals[j]);
    const u64 len = in_len(s, j);
    return group_hash_bytes(arr_at(s.bytes, s.vals[j], len), len);
}
// value j against a key: its 8 bytes, or its `len` bytes at p -- the length before any byte
SJ_HD bool in_value_is(const InSet &s, u32 j, u64 x, const u8 *p, u64 len) {
    if (s.kind != IN_KIND_STRING) return s.vals[j] == x;
    return in_len(s, j) == len && group_bytes_equal(arr_at(s.bytes, s.vals[j], len), p, len);
}
SJ_HD bool in_values_equal(const InSet &s, u32 a, u32 b) {
    if (s.kind != IN_KIND_STRING) return s.vals[a] == s.vals[b];
    const u64 len = in_len(s, b);
    return in_value_is(s, a, 0, arr_at(s.bytes, s.vals[b], len), len);
}

// Value j, whose hash is h, takes its place: k_q_group_insert's loop.  An empty slot is claimed; an occupied one is compared BY
// VALUE (the values were all there before the build began; hash[] of the occupant may not be yet) and on equality lowered to the
// smaller index; else the probe goes on.  The occupant of a slot only ever changes to a smaller index of an EQUAL value, so a
// comparison stays valid.  Nothing locks, nothing spins; the capacity exceeds the values, and the loop is bounded by it besides.
// T: load(cell), claim(cell, j) -> what the cell held (GROUP_NONE: claimed), lower(cell, j).  -> the slot value j ended in
template <typename T>
SJ_HD u32 in_insert(const InSet &s, u32 j, u64 h, T tab) {
    u32 slot = (u32)h & s.mask;
    for (u32 step = 0; step <= s.mask; step++, slot = (slot + 1u) & s.mask) {
        u32 *const cell = &s.table[slot];
        u32 cur = tab.load(cell);
        if (cur == GROUP_NONE) {
            cur = tab.claim(cell, j);
            if (cur == GROUP_NONE) break;
        }
        if (cur == j) break;
        if (in_values_equal(s, j, cur)) {
            if (cur > j) tab.lower(cell, j);
            break;
        }
    }
    return slot;
}
// Is the key -- hash h; its 8 bytes x, or its len bytes at p -- a value of the set?  From the home slot to the first empty one: the
// stored hash first, then the value.  (The table is complete: plain loads.)  *steps, if asked for: the slots looked at.
SJ_HD bool in_probe(const InSet &s, u64 h, u64 x, const u8 *p, u64 len, u32 *steps = nullptr) {
    u32 slot = (u32)h & s.mask;
    bool found = false;
    u32 step = 0;
    for (; step <= s.mask; step++, slot = (slot + 1u) & s.mask) {
        const u32 cur = s.table[slot];
        if (cur == GROUP_NONE) break;
        if (s.hash[cur] == h && in_value_is(s, cur, x, p, len)) {
            found = true;
            break;
        }
    }
    if (steps) *steps = step + 1u;
    return found;
}

// the table of the replay and of any serial caller
struct InPlainTable {
    SJ_HD u32 load(u32 *cell) const { return *cell; }
    SJ_HD u32 claim(u32 *cell, u32 j) const {
        const u32 was = *cell;
        if (was == GROUP_NONE) *cell = j;
        return was;
    }
    SJ_HD void lower(u32 *cell, u32 j) const {
        if (j < *cell) *cell = j;
    }
};

}  // namespace sj
