// sj_tablewalk.h -- the walk of a table (sj_table.h): every column of ONE record resolved to a tape index or a path status in one
// pass over the record's members.  The walk starts at the tape index of a value -- `root`: the root value of a record, or the value
// of a row of a row selection (query.hip row_value) -- and never looks in front of it.  Host and device: k_q_table_walk (query.hip) runs it with one lane per record, and
// host_selftest.cpp replays it over an oracle tape (sj_selftest_table_walk, tests/test_table_walk.py).
//
// FindElement's rules hold for every column on its own: into the root and into objects, not into arrays; at every level the first
// member with the key wins, and nothing is taken back -- a node that has been matched is never matched again, so a later member
// with the same key is passed over, whatever the first one's value was.  Per member of the object the walk stands in:
//   the key is compared with the children of the current node that are not matched yet (lengths first);
//   on a match the child is marked, and the columns that end at it get the index of the member's value;
//   a child with children of its own is entered at once when the value is an object -- the scan of the parent resumes behind it
//   when it is finished -- and is NOT_OBJECT for everything below it when the value is anything else;
//   the scan of an object ends when all the node's children are matched, the record when nothing is open any more.
// What is not matched at the end is NOT_FOUND, or NOT_OBJECT below a value that was no object (and everywhere when the root is none).
//
// State: the matched and the not-an-object nodes are two 32-bit masks; the resume stack -- the end and the node of every object
// that is open around the current one, at most 15 -- lies behind a pointer, two u32 per level `stride` words apart (LDS on the
// device, one column per lane; a local array on the host), the ends relative to `root`.  Nothing is an array
// indexed per lane in registers.
//   View:  u64 word(u64 i)                                        the tape
//          bool key_equals(u64 kw, u64 kl, u32 key_b, u32 key_n)  the string (kw, kl) equals plan key bytes [key_b, key_b + key_n)
//   Sink:  void operator()(u32 column, u64 v)                     exactly once per column: a tape index or SJHIP_PATH_NOT_*
#pragma once
#include "../../include/sjhip.h"
#include "sj_chunk.h"
#include "sj_table.h"

namespace sj {

static constexpr int TABLE_STACK_WORDS = 2 * TABLE_MAX_PATH;  // per record

SJ_HD u32 table_children(const TablePlan &pl, u32 node) {  // the mask of the node's children
    const u32 b = node == TABLE_ROOT ? 0u : pl.child_b[node], n = node == TABLE_ROOT ? pl.root_n : pl.child_n[node];
    return (u32)(((1ull << n) - 1ull) << b);
}

template <class View, class Sink>
SJ_HD void table_walk(const View &q, const TablePlan &pl, u64 root, u32 *stack, u32 stride, Sink &emit) {
    const u64 PAYLOAD = 0x00ffffffffffffffull;
    u32 matched = 0, notobj = 0;
    const u64 w = q.word(root);
    if ((u32)(w >> 56) != (u32)'{') {
        notobj = ~0u;
    } else {
        u64 end = (w & PAYLOAD) - 1;  // index of the closing '}'
        u64 i = root + 1;
        u32 cur = TABLE_ROOT, todo = table_children(pl, cur), sp = 0;
        for (;;) {
            if (i >= end || (todo & ~matched) == 0) {  // this object is finished: behind it in the one around it
                if (sp == 0) break;
                sp--;
                i = end + 1;
                end = root + stack[(2 * sp) * stride];
                cur = stack[(2 * sp + 1) * stride];
                todo = table_children(pl, cur);
                continue;
            }
            const u64 kw = q.word(i), kl = q.word(i + 1);  // member key
            const u64 v = i + 2, vw = q.word(v);
            const u32 vt = (u32)(vw >> 56);
            u32 hit = TABLE_ROOT;
            for (u32 rest = todo & ~matched; rest; rest &= rest - 1) {
                const u32 j = (u32)__builtin_ctz(rest);
                const u32 b = j ? pl.key_end[j - 1] : 0u;
                if (q.key_equals(kw, kl, b, pl.key_end[j] - b)) {
                    hit = j;
                    break;
                }
            }
            if (hit != TABLE_ROOT) {
                matched |= 1u << hit;
                for (u32 cs = pl.cols[hit]; cs; cs &= cs - 1) emit((u32)__builtin_ctz(cs), v);
                if (pl.child_n[hit]) {
                    if (vt == (u32)'{') {
                        stack[(2 * sp) * stride] = (u32)(end - root);
                        stack[(2 * sp + 1) * stride] = cur;
                        sp++;
                        cur = hit;
                        todo = table_children(pl, cur);
                        end = (vw & PAYLOAD) - 1;
                        i = v + 1;
                        continue;
                    }
                    notobj |= pl.sub[hit];
                }
            }
            // behind the member's value
            if (vt == (u32)'{' || vt == (u32)'[') i = vw & PAYLOAD;
            else i = (vt == (u32)'"' || vt == (u32)'l' || vt == (u32)'u' || vt == (u32)'d') ? v + 2 : v + 1;
        }
    }
    for (u32 rest = ~matched & (u32)((1ull << pl.n_nodes) - 1ull); rest; rest &= rest - 1) {
        const u32 j = (u32)__builtin_ctz(rest);
        const u64 st = ((notobj >> j) & 1u) ? SJHIP_PATH_NOT_OBJECT : SJHIP_PATH_NOT_FOUND;
        for (u32 cs = pl.cols[j]; cs; cs &= cs - 1) emit((u32)__builtin_ctz(cs), st);
    }
}

}  // namespace sj
