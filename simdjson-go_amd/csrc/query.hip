// query.hip -- queries over the DEVICE-RESIDENT result of the last parse of a context.
//
// The tape is up to 1.7x the input and PCIe moves ~55 GB/s, so a parse whose result has to cross to the host is
// D2H-bound by more than 10x; what callers of ParseND usually want is an aggregate or a subset of the records:
//     countWhere("Make", "HOND", pj)                      ndjson_test.go:421-471 (README example :226-269)
//     Object.FindKey(key) per record + string compare     parsed_object.go:97-138
// sjhip_count_where evaluates exactly that on the device and returns 8 bytes; sjhip_filter_where compacts the
// matching records into a new, self-contained (Tape, Strings.B) on the device -- bit-identical to what ParseND
// produces for the document made of the matching lines -- so that only the subset crosses PCIe.
// sjhip_filter_rows does the same for the rows of the row selection (sjhip_select_rows / sjhip_where_path): any predicate, rows
// inside arrays, one root per row.
//
// Semantics of a match (the reference's countWhere): the record's root value is an object; the FIRST member of that
// object whose key equals `key` (top level only, FindKey does not descend) has a string value equal to `value`.
// Strings are compared after unescaping (they are read from Strings.B / the message exactly as the Iter API does).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <array>
#include <vector>

#include "../../include/sjhip.h"
#include "sj_ctx.h"
#include "sj_device.h"
#include "sj_bounds.h"
#include "sj_ftoa.h"
#include "sj_group.h"
#include "sj_order.h"
#include "sj_sort.h"
#include "sj_stage2.h"
#include "sj_tapewalk.h"
#include "sj_tablewalk.h"
#include "sj_where.h"
#include "sj_wherein.h"

using namespace sj;

namespace {

static constexpr u32 NONE32 = 0xffffffffu;
static constexpr int QMAX = 1024;  // longest key / value a query may name (they travel as kernel arguments)

// (Arr: sj_bounds.h -- a plain pointer in the product build; in the debug build (-DSJ_DEBUG_BOUNDS) every index that comes out
// of a tape word -- the end of a container, the offset and length of a string -- is checked against the array it is used on,
// and a violation fails the query instead of reading outside the arenas)
struct QView {
    Arr<const u64> tape;
    u64 tape_len;
    Arr<const u8> strings;
    u64 strings_len;
    Arr<const u8> msg; // device copy of the message (strings that were not copied point into it)
    u64 msg_len;
    Arr<const u32> nl_off; // tape offset (inside this context's tape) of the close root of record r (r < R)
    u32 R;             // record-separating newline runs: R + 1 records
    // A shard of a sharded ParseND (parse_nd_big: an ND message beyond one context's reach) stores its indices in the MERGED index
    // space: tape indices + tape_base, Strings.B offsets + the shard's Strings.B base, message offsets + its message base.  The view
    // of such a shard holds `tape`, `strings` and `msg` as pointers moved DOWN by those bases, so that every index a tape word holds
    // -- and every index the path queries hand out -- is used as it stands; only the record bounds (nl_off: local) add tape_base.
    u64 tape_base;     // 0 for an unsharded result; tape_len: END of this context's stretch in the merged index space
    // The row selection of the context (sjhip_select_rows): the tape index of the value of every row of this part, in document
    // order.  Null: there is none, and the rows of a query are the records.  The filter and countWhere never see it (make_view).
    Arr<const u64> rows;
    u64 n_rows;
    u8 key[QMAX], val[QMAX];
    u32 klen, vlen;
};

__device__ __forceinline__ u64 rec_open(const QView &q, u32 r) { return q.tape_base + (r == 0 ? 0u : q.nl_off[r - 1] + 1u); }
__device__ __forceinline__ u64 rec_close(const QView &q, u32 r) { return r == q.R ? q.tape_len - 1u : q.tape_base + q.nl_off[r]; }
// what a path query runs on: the rows of the selection, or the records -- how many there are, and the tape index of the value of
// row r: the row's element, or the record's root value
__device__ __forceinline__ u32 q_rows(const QView &q) { return q.rows ? (u32)q.n_rows : q.R + 1u; }
__device__ __forceinline__ u64 row_value(const QView &q, u32 r) { return q.rows ? q.rows[r] : rec_open(q, r) + 1u; }

__device__ __forceinline__ const u8 *str_bytes(const QView &q, u64 word, u64 len) {
    const u64 p = word & TW_PAYLOAD;
    return (p & STRINGBUFBIT) ? arr_at(q.strings, p & (STRINGBUFBIT - 1), len) : arr_at(q.msg, p, len);
}
__device__ __forceinline__ bool str_equals(const QView &q, u64 word, u64 len, const u8 *want, u32 wlen) {
    if (len != wlen) return false;
    const u8 *s = str_bytes(q, word, len);
    for (u32 k = 0; k < wlen; k++)
        if (s[k] != want[k]) return false;
    return true;
}

// ---- paths, typed values, key sets (round 5: Iter.FindElement parsed_json.go:833-865, Object.FindPath parsed_object.go:256-313,
// Object.ForEach with onlyKeys parsed_object.go:142-196) ----------------------------------------------------------------------
// The keys of a path / of a key set travel concatenated in QView::key; QPath holds where each one ends.
static constexpr int QPATH_MAX = 16;
struct QPath {
    u32 end[QPATH_MAX];  // key j = key[end[j - 1] .. end[j])
    u32 n;
};
__device__ __forceinline__ bool key_is(const QView &q, const QPath &pth, u32 j, u64 word, u64 len) {
    const u32 b = j ? pth.end[j - 1] : 0u;
    return str_equals(q, word, len, q.key + b, pth.end[j] - b);
}
__device__ __forceinline__ u64 skip_value(u64 v, u64 vw) {  // index behind the value whose first word is vw = tape[v]
    const u32 vt = (u32)(vw >> 56);
    if (vt == '{' || vt == '[') return vw & TW_PAYLOAD;  // behind the matching close
    return two_word_tag(vw) ? v + 2 : v + 1;
}
// FindElement on row r (record r without a row selection): into the root, into objects, not into arrays; the first member with the key wins at every
// level.  Returns the tape index of the element's value, SJHIP_PATH_NOT_FOUND (ErrPathNotFound) or SJHIP_PATH_NOT_OBJECT
// ("type ... found before object was found" / "value of key ... is not an object").
__device__ u64 record_find_path(const QView &q, const QPath &pth, u32 r) {
    const u64 o = row_value(q, r);
    const u64 w = q.tape[o];
    if ((w >> 56) != '{') return SJHIP_PATH_NOT_OBJECT;
    u64 end = (w & TW_PAYLOAD) - 1;  // index of the closing '}'
    u64 i = o + 1;
    u32 seg = 0;
    while (i < end) {
        const u64 kw = q.tape[i], kl = q.tape[i + 1];  // member key
        const u64 v = i + 2, vw = q.tape[v];           // (asked for with the key, as countWhere's walk always did: one round trip per member)
        if (key_is(q, pth, seg, kw, kl)) {
            if (seg + 1 == pth.n) return v;
            if ((vw >> 56) != '{') return SJHIP_PATH_NOT_OBJECT;
            end = (vw & TW_PAYLOAD) - 1;
            i = v + 1;
            seg++;
            continue;
        }
        i = skip_value(v, vw);
    }
    return SJHIP_PATH_NOT_FOUND;
}
// what Iter.Float / Int / Uint / Bool return for the element whose first word is tape[v] (parsed_json.go:560-749, 867-875:
// integers, unsigned integers and floats convert into each other where the value fits): SJHIP_COL_OK with the value's bits
// in *out, or the error the reference returns (SJHIP_COL_NULL for null, SJHIP_COL_TYPE for the other types)
__device__ __forceinline__ int element_to(const QView &q, u64 v, int kind, u64 *out) {
    const u64 w = q.tape[v];
    const u32 t = (u32)(w >> 56);
    *out = 0;
    if (t == 'n') return SJHIP_COL_NULL;
    if (kind == SJHIP_COL_BOOL) {
        if (t != 't' && t != 'f') return SJHIP_COL_TYPE;
        *out = t == 't';
        return SJHIP_COL_OK;
    }
    if (t != 'l' && t != 'u' && t != 'd') return SJHIP_COL_TYPE;
    const u64 raw = q.tape[v + 1];
    const double d = __longlong_as_double((long long)raw);
    if (kind == SJHIP_COL_FLOAT) {
        *out = t == 'd' ? raw : (u64)__double_as_longlong(t == 'l' ? (double)(long long)raw : (double)raw);
        return SJHIP_COL_OK;
    }
    if (kind == SJHIP_COL_INT) {
        if (t == 'l') *out = raw;
        else if (t == 'u') {
            if (raw > 0x7fffffffffffffffull) return SJHIP_COL_RANGE;
            *out = raw;
        } else {
            // an error above math.MaxInt64 / below math.MinInt64 (as float64 constants: 2^63 and -2^63), else int64(v) -- which
            // for v == 2^63 is the amd64 conversion's "integer indefinite", MinInt64
            if (d > 9223372036854775808.0 || d < -9223372036854775808.0) return SJHIP_COL_RANGE;
            *out = d >= 9223372036854775808.0 || d != d ? 0x8000000000000000ull : (u64)(long long)d;
        }
        return SJHIP_COL_OK;
    }
    // SJHIP_COL_UINT
    if (t == 'u') *out = raw;
    else if (t == 'l') {
        if ((long long)raw < 0) return SJHIP_COL_RANGE;
        *out = raw;
    } else {
        // an error only for v > math.MaxUint64 -- which as a float64 constant is 2^64 -- and for v < 0; uint64(v) of exactly 2^64
        // is the amd64 conversion's result: (v - 2^63) converts to the integer indefinite 0x8000000000000000, XORed with the sign
        // bit = 0 (the mirror image of the INT edge at 2^63)
        if (d != d) *out = 0x8000000000000000ull;  // NaN never reaches the tape (parse_number rejects it); amd64: indefinite
        else if (d < 0.0 || d > 18446744073709551616.0) return SJHIP_COL_RANGE;
        else *out = d >= 18446744073709551616.0 ? 0ull : (u64)d;
    }
    return SJHIP_COL_OK;
}
// the ordering comparisons and the prefix test (SJHIP_OP_LT_INT .. SJHIP_OP_PREFIX_STRING), apart from the switch of the
// equalities below, whose code they leave as it was: the element converted as the EQ_* operator of its kind converts it -- an
// element whose conversion is not OK satisfies nothing --, then Go's comparison of two int64 / uint64 / float64 (a NaN `want`
// compares false with everything); PREFIX_STRING: bytes.HasPrefix(Iter.StringBytes, value)
__device__ __forceinline__ bool element_orders(const QView &q, u64 v, int op, u64 want, const u8 *val, u32 vlen) {
    if (op == SJHIP_OP_PREFIX_STRING) {
        const u64 w = q.tape[v];
        if ((u32)(w >> 56) != '"') return false;
        const u64 len = q.tape[v + 1];
        if (len < vlen) return false;
        const u8 *s = str_bytes(q, w, vlen);
        for (u32 k = 0; k < vlen; k++)
            if (s[k] != val[k]) return false;
        return true;
    }
    if (op < SJHIP_OP_LT_INT || op > SJHIP_OP_GE_FLOAT) return false;
    const int o = op - SJHIP_OP_LT_INT, rel = o & 3;  // rel: < <= > >=
    const int kind = o < 4 ? SJHIP_COL_INT : (o < 8 ? SJHIP_COL_UINT : SJHIP_COL_FLOAT);
    u64 got;
    if (element_to(q, v, kind, &got) != SJHIP_COL_OK) return false;
    bool lt, gt;
    if (kind == SJHIP_COL_INT) lt = (long long)got < (long long)want, gt = (long long)got > (long long)want;
    else if (kind == SJHIP_COL_UINT) lt = got < want, gt = got > want;
    else {
        const double a = __longlong_as_double((long long)got), b = __longlong_as_double((long long)want);
        if (a != a || b != b) return false;
        lt = a < b, gt = a > b;
    }
    return rel == 0 ? lt : (rel == 1 ? !gt : (rel == 2 ? gt : !lt));
}
// the typed comparisons: the element converted as above (StringBytes for EQ_STRING), compared with the wanted value -- a number or
// a bool in `want`, a string in val[0 .. vlen)
__device__ bool element_is(const QView &q, u64 v, int op, u64 want, const u8 *val, u32 vlen) {
    const u64 w = q.tape[v];
    const u32 t = (u32)(w >> 56);
    u64 got;
    switch (op) {
    case SJHIP_OP_EXISTS: return true;
    case SJHIP_OP_EQ_STRING: return t == '"' && str_equals(q, w, q.tape[v + 1], val, vlen);
    case SJHIP_OP_EQ_BOOL: return element_to(q, v, SJHIP_COL_BOOL, &got) == SJHIP_COL_OK && got == (want != 0);
    case SJHIP_OP_IS_NULL: return t == 'n';
    case SJHIP_OP_EQ_INT: return element_to(q, v, SJHIP_COL_INT, &got) == SJHIP_COL_OK && got == want;
    case SJHIP_OP_EQ_UINT: return element_to(q, v, SJHIP_COL_UINT, &got) == SJHIP_COL_OK && got == want;
    case SJHIP_OP_EQ_FLOAT:  // (a comparison of doubles: -0.0 equals 0.0)
        return element_to(q, v, SJHIP_COL_FLOAT, &got) == SJHIP_COL_OK &&
               __longlong_as_double((long long)got) == __longlong_as_double((long long)want);
    default: return element_orders(q, v, op, want, val, vlen);
    }
}
// (one predicate per call: its string value is the whole of QView::val)
__device__ __forceinline__ bool element_is(const QView &q, u64 v, int op, u64 want) { return element_is(q, v, op, want, q.val, q.vlen); }
// the record's element at the path exists and satisfies the predicate
__device__ __forceinline__ bool record_is(const QView &q, const QPath &pth, u32 r, int op, u64 want) {
    const u64 v = record_find_path(q, pth, r);
    return v < SJHIP_PATH_NOT_OBJECT && element_is(q, v, op, want);
}
// one atomic per wave: the lanes whose record counts
__device__ __forceinline__ void count_ballot(bool m, unsigned long long *count) {
    const u64 b = __ballot(m);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(count, (unsigned long long)__popcll(b));
}

// ---- filter: pass 1, one lane per record ------------------------------------------------------------------------
struct QRec {
    u32 *flag;      // [R+1] 1 if the record matches
    u32 *words;     // [R+1] its tape words if it matches, else 0      -> exclusive prefix = new index of its open root
    u32 *first_str; // [R+1] Strings.B offset of its first string, NONE32 if it has none
    u32 *s_len;     // [R+1] bytes of Strings.B a matching record owns (pass 2)
    u32 *s_pre;     // [R+1] their exclusive prefix = new Strings.B offset of its first string (pass 2)
    unsigned long long *totals;  // matching records, tape words, Strings.B bytes
};
// (key: the one-key path of countWhere(key, value), whose match is FindElement + the string compare)
__global__ __launch_bounds__(256) void k_q_mark(QView q, QPath key, QRec o) {
    const u32 r = blockIdx.x * 256 + threadIdx.x;
    if (r > q.R) return;
    const bool m = record_is(q, key, r, SJHIP_OP_EQ_STRING, 0);
    const u32 a = rec_open(q, r), c = rec_close(q, r);
    o.flag[r] = m ? 1u : 0u;
    o.words[r] = m ? c - a + 1u : 0u;
    // first string of the record: walk its items, into the containers (a number's second word is raw data and is stepped over)
    u32 fs = NONE32;
    for (u64 i = (u64)a + 1; i < c;) {
        const u64 w = q.tape[i];
        if ((w >> 56) == '"') {
            fs = (u32)(w & (STRINGBUFBIT - 1));  // every string is copied (checked by the host): a Strings.B offset
            break;
        }
        i += two_word_tag(w) ? 2 : 1;
    }
    o.first_str[r] = fs;
}

// ---- pass 2: exclusive prefixes of words / string bytes over the records, and the Strings.B range of every record:
// [its first string, the first string of any later record) -- strings are laid out in document order, so "the first
// string of any later record" is a minimum over the records behind it.  Tiles of 1024 records (256 threads x 4
// consecutive records), tile sums scanned by one block (sj_tapewalk.h), then applied: sums -> scans -> apply (word
// prefixes, string lengths and their tile sums) -> scan -> apply (string prefixes).
struct QTiles {
    unsigned long long *tw;  // [tiles] tape words of the tile's matching records -> their exclusive prefix
    unsigned long long *tb;  // [tiles] Strings.B bytes of the tile's matching records -> their exclusive prefix
    unsigned long long *tc;  // [tiles] matching records of the tile
    // [tiles] entry tiles - 1 - t: NONE32 - the first string of tile t (0: it has none).  "The first string of any later tile" is
    // a minimum over the tiles behind t; mirrored and complemented it is the exclusive running maximum k_tw_scan_last computes
    // (-1 for the last tile: no tile behind it).
    long long *tf;
};
// minimum over the threads behind this one (NONE32 if there is none)
__device__ __forceinline__ u32 q_block_excl_suffix_min(u32 v, u32 *s_w, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    u32 incl = v;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const u32 o = (u32)__shfl_down((int)incl, s, 64);
        if (lane + s < 64) incl = o < incl ? o : incl;
    }
    if (lane == 0) s_w[wave] = incl;
    __syncthreads();
    u32 after = NONE32;
    for (int w = 0; w < QT / 64; w++)
        if (w > wave) after = s_w[w] < after ? s_w[w] : after;
    u32 ex = (u32)__shfl_down((int)incl, 1, 64);
    if (lane == 63) ex = NONE32;
    __syncthreads();
    return ex < after ? ex : after;
}
// tile sums of words and flags, and the tile's first string (mirrored: QTiles::tf)
__global__ __launch_bounds__(QT) void k_q_tile_sums(QRec o, u32 n, QTiles T) {
    __shared__ long long s_l[QT / 64];
    const int tid = threadIdx.x;
    tile_sums(o.words, n, T.tw);
    tile_sums(o.flag, n, T.tc);
    u32 f[QI], mn = NONE32;
    (void)q_load4(o.first_str, n, NONE32, f);
#pragma unroll
    for (int k = 0; k < QI; k++) mn = f[k] < mn ? f[k] : mn;
    const long long mine = (long long)(NONE32 - mn), before = block_excl_max(mine, s_l, tid);
    if (tid == QT - 1) T.tf[gridDim.x - 1 - blockIdx.x] = before > mine ? before : mine;  // the block's maximum
}

// words[r] := new index of the record's open root; s_len[r]; tile sums of s_len
__global__ __launch_bounds__(QT) void k_q_tile_apply1(QRec o, u32 n, QTiles T, u32 strings_len) {
    __shared__ unsigned long long s_w[QT / 64];
    __shared__ u32 s_m[QT / 64];
    const int tid = threadIdx.x;
    const u32 base = blockIdx.x * QTILE + (u32)tid * QI;
    u32 w[QI], fl[QI], f[QI];
    const unsigned long long tw = q_load4(o.words, n, 0u, w);
    (void)q_load4(o.flag, n, 0u, fl);
    (void)q_load4(o.first_str, n, NONE32, f);
    u32 mn = NONE32;
#pragma unroll
    for (int k = 0; k < QI; k++) mn = f[k] < mn ? f[k] : mn;
    unsigned long long pw = T.tw[blockIdx.x] + block_excl_sum(tw, s_w, tid, nullptr);
    const long long later_tiles = T.tf[gridDim.x - 1 - blockIdx.x];
    u32 behind_tile = later_tiles < 0 ? NONE32 : NONE32 - (u32)later_tiles;  // first string of any later tile ...
    behind_tile = behind_tile < strings_len ? behind_tile : strings_len;     // ... or the end of Strings.B
    const u32 later = q_block_excl_suffix_min(mn, s_m, tid);
    u32 nxt = later < behind_tile ? later : behind_tile;  // first string of any record behind this thread's four
    u32 len[QI];
    unsigned long long tb = 0;
#pragma unroll
    for (int k = QI - 1; k >= 0; k--) {
        u32 l = 0;
        if (f[k] != NONE32) {
            l = nxt - f[k];
            nxt = f[k];
        }
        len[k] = fl[k] ? l : 0u;
        tb += len[k];
    }
#pragma unroll
    for (int k = 0; k < QI; k++) {
        if (base + k < n) {
            o.words[base + k] = (u32)pw;
            o.s_len[base + k] = len[k];
        }
        pw += w[k];
    }
    unsigned long long tot_b = 0;
    (void)block_excl_sum(tb, s_w, tid, &tot_b);
    if (tid == 0) T.tb[blockIdx.x] = tot_b;
}

// s_pre[r] := new Strings.B offset of the record's first string
__global__ __launch_bounds__(QT) void k_q_tile_apply2(QRec o, u32 n, QTiles T) { tile_apply(o.s_len, o.s_pre, n, T.tb); }

// ---- pass 3: one wave per record: its tape words with every stored index rebased, then its strings -------------------
// The rebasing copy of both filters (k_q_copy, k_q_frows_copy): a stretch of tape becomes a self-contained record.  By one wave
// (all arguments wave-uniform): the nwords words of the value at v -- the first word of an entry, as tw_walk_span asks -- go to
// out_tape[na + 1 ..) between two synthesised roots at na and na + nwords + 1; bracket payloads move by (new index - old index),
// string payloads by (new offset - old offset), raw words (told by the span walk of sj_tapewalk.h) stay as they are.  Then the
// slen bytes of Strings.B the value owns go from sb to ns, 64 at a time.
__device__ __forceinline__ void wave_copy_record(const QView &q, u64 v, u64 nwords, u64 na, u32 sb, u32 slen, u32 ns, int lane,
                                                 Arr<u64> out_tape, Arr<u8> out_strings) {
    const long long dw = (long long)(na + 1) - (long long)v;
    const u64 ds = (u64)((long long)ns - (long long)sb);  // only used when the value has a string
    if (lane == 0) {
        out_tape[na] = ((u64)'r' << 56) | (na + nwords + 2);  // behind its closing root: the next record, or the tape length
        out_tape[na + nwords + 1] = ((u64)'r' << 56) | na;
    }
    tw_walk_span(q.tape, v, nwords, lane, [&](u64 i, u64 w, bool in, bool raw) {
        if (!in) return;
        const u32 t = (u32)(w >> 56);
        u64 x = w;
        if (!raw) {
            if (t == '{' || t == '[' || t == '}' || t == ']') x = (w & ~TW_PAYLOAD) | (u64)((long long)(w & TW_PAYLOAD) + dw);
            else if (t == '"') x = w + ds;
        }
        out_tape[na + 1 + i] = x;
    });
    for (u32 k = (u32)lane; k < slen; k += 64) out_strings[(u64)ns + k] = q.strings[(u64)sb + k];
}
__global__ __launch_bounds__(256) void k_q_copy(QView q, QRec o, Arr<u64> out_tape, Arr<u8> out_strings) {
    const u32 r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r > q.R || !o.flag[r]) return;  // wave-uniform
    const u64 a = rec_open(q, r), c = rec_close(q, r);
    wave_copy_record(q, a + 1, c - a - 1, o.words[r], o.first_str[r], o.s_len[r], o.s_pre[r], threadIdx.x & 63, out_tape, out_strings);
}

// ---- the kernels of the path queries ------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_q_find_path(QView q, QPath pth, u64 *out) {
    const u32 r = blockIdx.x * 256 + threadIdx.x;
    if (r < q_rows(q)) out[r] = record_find_path(q, pth, r);
}
__global__ __launch_bounds__(256) void k_q_count_path(QView q, QPath pth, int op, u64 want, unsigned long long *count) {
    const u32 r = blockIdx.x * 256 + threadIdx.x;
    count_ballot(r < q_rows(q) && record_is(q, pth, r, op, want), count);
}
// ForEach(fn, onlyKeys) on the root object of record r: the members whose key is in the set, in document order, until as
// many members as the set has keys have been delivered (parsed_object.go:190-194: a key that occurs twice counts twice).
// out[r * n + j] = key number << 56 | tape index of the value of the j-th delivered member; ~0: no further member
__global__ __launch_bounds__(256) void k_q_project(QView q, QPath set, u64 *out) {
    const u32 r = blockIdx.x * 256 + threadIdx.x;
    if (r >= q_rows(q)) return;
    u64 *dst = out + (u64)r * set.n;
    u32 n = 0;
    const u64 o = row_value(q, r);
    const u64 w = q.tape[o];
    if ((w >> 56) == '{') {
        const u64 end = (w & TW_PAYLOAD) - 1;
        for (u64 i = o + 1; i < end && n < set.n;) {
            const u64 v = i + 2;
            for (u32 j = 0; j < set.n; j++)
                if (key_is(q, set, j, q.tape[i], q.tape[i + 1])) {
                    dst[n++] = ((u64)j << 56) | v;
                    break;
                }
            i = skip_value(v, q.tape[v]);
        }
    }
    for (; n < set.n; n++) dst[n] = ~0ull;
}

// ---- columns: the value at a path of every record, converted (sjhip_extract_path / sjhip_extract_path_strings) -------------
// Numbers and bools: one lane per record -- FindElement, the conversion of element_to, one store of the value and one of the
// status; nothing is scanned.
__device__ __forceinline__ int path_status(u64 v) {
    return v == SJHIP_PATH_NOT_FOUND ? SJHIP_COL_NOT_FOUND : SJHIP_COL_NOT_OBJECT;
}
// the value at the path of row `row` (no keys: the row's own value) as a number of `kind`: its status, and its bits in *x
__device__ __forceinline__ int row_number(const QView &q, const QPath &pth, u32 row, int kind, u64 *x) {
    const u64 v = pth.n ? record_find_path(q, pth, row) : row_value(q, row);
    *x = 0;
    return v < SJHIP_PATH_NOT_OBJECT ? element_to(q, v, kind, x) : path_status(v);
}
__global__ __launch_bounds__(256) void k_q_extract(QView q, QPath pth, int kind, void *values, u8 *status) {
    const u32 r = blockIdx.x * 256 + threadIdx.x;
    if (r >= q_rows(q)) return;
    const u64 v = record_find_path(q, pth, r);
    u64 x = 0;
    const int st = v < SJHIP_PATH_NOT_OBJECT ? element_to(q, v, kind, &x) : path_status(v);
    if (kind == SJHIP_COL_BOOL) ((u8 *)values)[r] = (u8)x;
    else ((u64 *)values)[r] = x;
    status[r] = (u8)st;
}

// ---- aggregates: count, sum, min, max of that column, in all and per record (sjhip_aggregate_path / _aggregate_path_records) -----
// The reduction of what k_q_extract would write, without writing it: one lane per row walks and converts as above, and what
// leaves the lane is a partial -- OK and other rows counted, the sum, the smallest and the largest key -- that is reduced
// SEGMENTED by the record that owns the row.  The records are told by flags, not searched for: a row is the HEAD of a segment if
// it is the first row of its record and its END if the next row is a head (or there is none), so a selection of one record owning
// every row and one of a million records owning one row each are the same input.  The total is the same reduction with one
// segment over all rows (AGG_ONE); without a selection every row is its own segment and is stored as it is (AGG_OWN).
//   k_q_agg_heads   (AGG_OFFS) one lane per record: head[row_offsets[r]] = r + 1 for every record that has rows (head[] starts as 0;
//                   the outputs start as 0 as well, which is the answer for a record without rows)
//   k_q_agg_rows    per tile of AGG_TILE rows: the walk, then agg_tile: a segmented scan by wave shuffles (a head restarts the
//                   running partial), the waves joined in wave order through LDS.  A segment that begins and ends inside the tile
//                   is stored at its end row; what the tile cannot finish becomes at most two ITEMS of the next level: slot A, the
//                   piece of a segment that began in an earlier tile (it ends here, or it covers the whole tile), and slot B, the
//                   piece of the segment left open at the tile's end, with its record
//   k_q_agg_fold    the same agg_tile over the items of the level below, AGG_TILE per block, until a level fits one tile: a B item
//                   is a head, an A item that ends its segment an end.  Every level shrinks by 128, a record that spans any number
//                   of tiles costs no lane more than one item per level, and the association of a float sum is fixed by the number
//                   of rows and the offsets alone.
// Sums: FLOAT is IEEE double addition in that association (identity -0.0, no atomics).  INT / UINT are exact: a value travels as
// its low and its high 32-bit half (the high half signed for INT), each summed in 64 bits -- exact for 2^32 rows -- and put together
// as a 128-bit number where a segment is stored.  Min / max compare keys: a uint64 whose unsigned order is the order of the kind
// (INT: the sign bit flipped; FLOAT: all bits of a negative value flipped, the sign bit of the others: -0.0 below +0.0).
// The status histogram of the total is six ballots per wave and one integer atomic per status that occurs in it.
static constexpr int AGG_TILE = 256;
static_assert(ORDER_KIND_FLOAT == SJHIP_COL_FLOAT && ORDER_KIND_INT == SJHIP_COL_INT && ORDER_KIND_UINT == SJHIP_COL_UINT,
              "agg_key / agg_unkey (sj_order.h) take the column kinds");
enum : u32 { AGG_ONE = 0, AGG_OWN = 1, AGG_OFFS = 2 };        // QAgg::mode
enum : u32 { AGG_VALID = 1, AGG_HEAD = 2, AGG_END = 4 };      // AggItem::flags (0: no item)
struct AggVal {
    u32 ok, bad;  // rows whose conversion is SJHIP_COL_OK / is anything else
    u64 s0, s1;   // FLOAT: s0 = the bits of the sum; INT / UINT: the sums of the low / of the high halves
    u64 mn, mx;   // keys (agg_key); ~0 and 0 while no row is OK
};
struct AggItem {
    AggVal v;
    u32 rec1;     // the record of the segment + 1 (a head), else 0
    u32 flags;
};
struct QAgg {
    int kind;
    u32 mode;
    Arr<const u32> head;       // [rows] AGG_OFFS: record + 1 at the first row of every record that has rows, else 0
    Arr<AggItem> items;        // [2 * tiles] what this level hands to the next: slots A and B of every tile
    Arr<u64> out;              // six arrays of `records` entries end to end: count, not_ok, sum, sum_hi, min, max
    u64 records;
    unsigned long long *hist;  // [6] rows per status (the total), or null
    // the grouping (sjhip_group_path): position r of the reduction is row perm[r] of the view, and there are n_perm positions --
    // the rows that have a key, ordered by group.  Null: position r is row r, and there are as many as the view has rows.
    Arr<const u32> perm;
    u32 n_perm;
};
__device__ __forceinline__ AggVal agg_identity(bool flt) { return {0u, 0u, flt ? AGG_SIGN : 0ull, 0ull, ~0ull, 0ull}; }
// a: the rows in front, b: the rows behind
__device__ __forceinline__ AggVal agg_join(const AggVal &a, const AggVal &b, bool flt) {
    AggVal r;
    r.ok = a.ok + b.ok;
    r.bad = a.bad + b.bad;
    r.s0 = flt ? (u64)__double_as_longlong(__longlong_as_double((long long)a.s0) + __longlong_as_double((long long)b.s0)) : a.s0 + b.s0;
    r.s1 = a.s1 + b.s1;
    r.mn = a.mn < b.mn ? a.mn : b.mn;
    r.mx = a.mx > b.mx ? a.mx : b.mx;
    return r;
}
__device__ __forceinline__ AggVal agg_up(const AggVal &v, int s) {
    return {wave_up(v.ok, s), wave_up(v.bad, s), wave_up(v.s0, s), wave_up(v.s1, s), wave_up(v.mn, s), wave_up(v.mx, s)};
}
// the finished segment of record `rec`
__device__ __forceinline__ void agg_store(const QAgg &a, u64 rec, const AggVal &v) {
    u64 lo = 0, hi = 0;
    if (v.ok) {
        if (a.kind == SJHIP_COL_FLOAT) lo = v.s0;
        else {  // s0 + s1 * 2^32 in 128 bits
            lo = v.s0 + (v.s1 << 32);
            hi = (a.kind == SJHIP_COL_INT ? (u64)((long long)v.s1 >> 32) : v.s1 >> 32) + (lo < v.s0 ? 1u : 0u);
        }
    }
    a.out[rec] = v.ok;
    a.out[a.records + rec] = v.bad;
    a.out[2 * a.records + rec] = lo;
    a.out[3 * a.records + rec] = hi;
    a.out[4 * a.records + rec] = v.ok ? agg_unkey(v.mn, a.kind) : 0;
    a.out[5 * a.records + rec] = v.ok ? agg_unkey(v.mx, a.kind) : 0;
}
// One item per thread of the block, in item order.  Reduces every item with the items of its segment in front of it in the tile,
// stores the segments that begin and end here, and writes the tile's two slots of a.items.  An item that is not VALID -- a lane
// behind the last row, an empty slot of the level below -- is transparent: it adds the identity to whatever passes over it (slot
// B of a tile that lies wholly inside one segment is empty, and sits between that tile's slot A and the next one's).
__device__ __forceinline__ void agg_tile(const QAgg &a, AggVal v, u32 flags, u32 rec1, AggItem *s_tail /* [AGG_TILE / 64] */) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool flt = a.kind == SJHIP_COL_FLOAT;
    const bool valid = (flags & AGG_VALID) != 0, end = valid && (flags & AGG_END) != 0, last = tid == AGG_TILE - 1;
    // bit 0: a head among the items the partial covers -- it starts at its segment's first item; bits 1-2: the last valid item at
    // or in front of this one in the tile: 2 it leaves its segment open, 4 it ends it (0: none)
    u32 st = ((flags & AGG_HEAD) ? 1u : 0u) | (valid ? (end ? 4u : 2u) : 0u);
    u32 rk = rec1;  // the record + 1 of the last head at or in front of the item (they ascend); 0: none in the tile
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const AggVal o = agg_up(v, s);
        const u32 ost = wave_up(st, s), ork = wave_up(rk, s);
        if (lane >= s) {
            if (!(st & 1u)) v = agg_join(o, v, flt);
            st = ((st | ost) & 1u) | ((st & 6u) ? (st & 6u) : (ost & 6u));
            rk = ork > rk ? ork : rk;
        }
    }
    if (lane == 63) s_tail[wave] = {v, rk, st};
    __syncthreads();
    AggVal acc = agg_identity(flt);
    u32 ast = 0, ark = 0;
    for (int w = 0; w < AGG_TILE / 64; w++)
        if (w < wave) {
            const AggItem t = s_tail[w];
            acc = (t.flags & 1u) ? t.v : agg_join(acc, t.v, flt);
            ast = ((ast | t.flags) & 1u) | ((t.flags & 6u) ? (t.flags & 6u) : (ast & 6u));
            ark = t.rec1 > ark ? t.rec1 : ark;
        }
    if (!(st & 1u)) v = agg_join(acc, v, flt);
    st = ((st | ast) & 1u) | ((st & 6u) ? (st & 6u) : (ast & 6u));
    rk = ark > rk ? ark : rk;
    const bool f = (st & 1u) != 0, open = (st & 6u) == 2u;
    if (end && f) agg_store(a, (u64)rk - 1u, v);
    // slot A: the piece of a segment that began in an earlier tile -- it ends here, or it is still open behind the last item (the
    // whole tile); after an end the next valid item is a head, so at most one item of a tile goes there.  Slot B: the piece of
    // the segment that began here and is open behind the last item.
    const bool to_a = !f && (end || (last && open)), to_b = f && last && open;
    const AggItem none = {agg_identity(flt), 0u, 0u};
    if (to_a) a.items[2ull * blockIdx.x] = {v, 0u, AGG_VALID | (end ? (u32)AGG_END : 0u)};
    const int any_a = __syncthreads_or(to_a ? 1 : 0);
    if (tid == 0 && !any_a) a.items[2ull * blockIdx.x] = none;
    if (last) a.items[2ull * blockIdx.x + 1] = to_b ? AggItem{v, rk, AGG_VALID | AGG_HEAD} : none;
}
__global__ __launch_bounds__(256) void k_q_agg_heads(Arr<const u64> off, u32 records, Arr<u32> head) {
    const u32 r = blockIdx.x * 256 + threadIdx.x;
    if (r >= records) return;
    const u64 a = off[r];
    if (off[r + 1] > a) head[a] = r + 1u;
}
__global__ __launch_bounds__(AGG_TILE) void k_q_agg_rows(QView q, QPath pth, QAgg a) {
    __shared__ AggItem s_tail[AGG_TILE / 64];
    const u32 n = a.perm ? a.n_perm : q_rows(q), r = blockIdx.x * AGG_TILE + threadIdx.x;
    AggVal v = agg_identity(a.kind == SJHIP_COL_FLOAT);
    int st = -1;
    if (r < n) {
        const u32 row = a.perm ? a.perm[r] : r;
        u64 x;
        st = row_number(q, pth, row, a.kind, &x);
        if (st == SJHIP_COL_OK) {
            v.ok = 1;
            v.mn = v.mx = agg_key(x, a.kind);
            if (a.kind == SJHIP_COL_FLOAT) v.s0 = x;
            else {
                v.s0 = x & 0xffffffffull;
                v.s1 = a.kind == SJHIP_COL_INT ? (u64)((long long)x >> 32) : x >> 32;
            }
        } else v.bad = 1;
    }
    if (a.hist)
        for (int k = 0; k <= SJHIP_COL_RANGE; k++) count_ballot(st == k, &a.hist[k]);
    if (a.mode == AGG_OWN) {  // (block-uniform) record r owns row r
        if (r < n) agg_store(a, r, v);
        return;
    }
    u32 flags = 0, rec1 = 0;  // behind the last row: not VALID
    if (r < n) {
        if (a.mode == AGG_ONE) rec1 = r == 0 ? 1u : 0u;
        else rec1 = a.head[r];
        const bool end = r + 1 == n || (a.mode == AGG_OFFS && a.head[r + 1] != 0);
        flags = AGG_VALID | (rec1 ? (u32)AGG_HEAD : 0u) | (end ? (u32)AGG_END : 0u);
    }
    agg_tile(a, v, flags, rec1, s_tail);
}
// (a.items: the slots of THIS level; in: the m items of the level below)
__global__ __launch_bounds__(AGG_TILE) void k_q_agg_fold(QAgg a, Arr<const AggItem> in, u32 m) {
    __shared__ AggItem s_tail[AGG_TILE / 64];
    const u32 i = blockIdx.x * AGG_TILE + threadIdx.x;
    AggItem it = {agg_identity(a.kind == SJHIP_COL_FLOAT), 0u, 0u};
    if (i < m) it = in[i];
    agg_tile(a, it.v, it.flags, it.rec1, s_tail);
}

// Strings (Arrow's "large string" layout: u64 offsets, the bytes end to end) in three steps over the n = R + 1 records:
//   k_q_col_len      one lane per record: FindElement, the status, the length of the record's text and the tape index of the
//                    element (the gather does not walk the record again); entry n has length 0
//   scan             exclusive prefix of the n + 1 lengths in place (the filter's tile pattern: sums -> one-block scan -> apply),
//                    entry n = the total
//   k_q_col_gather   one lane per record: a number's text (StringCvt: at most 25 bytes) and a short string by the lane, a long
//                    string by the whole wave, 64 bytes at a time (strings run from 0 bytes to megabytes)
// A float's text is formatted twice -- its length in the first step (float_text_len: the counting form of the formatter), its
// bytes in the last -- instead of being stashed: the formatter is registers only, and a 32-byte stash for every record would
// cost more memory traffic than the float records' second formatting costs ALU time.
struct QCol {
    u64 *idx;                    // [n] tape index of the element
    u64 *off;                    // [n + 1] length of the record's text -> its offset in the column (entry n: the total)
    u8 *status;                  // [n]
    unsigned long long *tiles;   // [tiles] tile sums -> their exclusive prefix (k_tw_scan_sums)
};
// status and text length of what StringBytes (cvt = false) / StringCvt (parsed_json.go:775-800) return for tape[v]
__device__ __forceinline__ int element_text_len(const QView &q, u64 v, bool cvt, u64 *len) {
    const u32 t = (u32)(q.tape[v] >> 56);
    *len = 0;
    if (t == '"') {
        *len = q.tape[v + 1];
        return SJHIP_COL_OK;
    }
    if (!cvt) return t == 'n' ? SJHIP_COL_NULL : SJHIP_COL_TYPE;
    switch (t) {
    case 'l': *len = int_text_len(q.tape[v + 1]); return SJHIP_COL_OK;
    case 'u': *len = digit_count(q.tape[v + 1]); return SJHIP_COL_OK;
    case 'd': *len = float_text_len(q.tape[v + 1]); return *len ? SJHIP_COL_OK : SJHIP_COL_TYPE;  // (0: Inf / NaN, never on a tape)
    case 't': *len = 4; return SJHIP_COL_OK;
    case 'f': *len = 5; return SJHIP_COL_OK;
    case 'n': *len = 4; return SJHIP_COL_OK;
    }
    return SJHIP_COL_TYPE;  // { [
}
__global__ __launch_bounds__(256) void k_q_col_len(QView q, QPath pth, u32 cvt, QCol c) {
    const u32 r = blockIdx.x * 256 + threadIdx.x;
    if (r >= q_rows(q)) {
        if (r == q_rows(q)) c.off[r] = 0;
        return;
    }
    const u64 v = record_find_path(q, pth, r);
    u64 len = 0;
    const int st = v < SJHIP_PATH_NOT_OBJECT ? element_text_len(q, v, cvt != 0, &len) : path_status(v);
    c.idx[r] = v;
    c.off[r] = len;
    c.status[r] = (u8)st;
}
__global__ __launch_bounds__(QT) void k_q_col_tile_sums(QCol c, u32 m) { tile_sums(c.off, m, c.tiles); }
__global__ __launch_bounds__(QT) void k_q_col_tile_apply(QCol c, u32 m) { tile_apply(c.off, c.off, m, c.tiles); }
// out_off[0 .. n] (the part's own offsets, from 0), out_status[n], data: the column (d_col).  One lane per record for what is
// per record -- the offset, the status, a number's text (at most 25 bytes), a string of up to SHORT bytes -- and the whole wave
// for each longer string of its 64 records in turn, 64 bytes at a time (strings run from 0 bytes to megabytes).
static constexpr u64 COL_SHORT = 32;
__device__ __forceinline__ void copy_bytes(u8 *dst, const u8 *src, u64 len, u64 first, u64 step) {
    for (u64 k = first; k < len; k += step) dst[k] = src[k];
}
// the wave's long strings, one after another: the `len` bytes of the string whose tag word is w, to data[o ..), for every lane with `wide`
__device__ __forceinline__ void wave_copy_strings(const QView &q, Arr<u8> data, bool wide, u64 o, u64 len, u64 w, int lane) {
    wave_each(wide, [&](int j) {
        const u64 oj = wave_bcast(o, j), lj = wave_bcast(len, j);
        copy_bytes(arr_at(data, oj, lj), str_bytes(q, wave_bcast(w, j), lj), lj, (u64)lane, 64);
    });
}
__global__ __launch_bounds__(256) void k_q_col_gather(QView q, QCol c, u64 *out_off, u8 *out_status, Arr<u8> data) {
    const u32 r = blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    u64 o = 0, len = 0, w = 0;
    bool wide = false;
    if (r < q_rows(q)) {
        o = c.off[r];
        len = c.off[r + 1] - o;
        const u8 st = c.status[r];
        out_off[r] = o;
        out_status[r] = st;
        if (r + 1 == q_rows(q)) out_off[r + 1] = o + len;
        if (st == SJHIP_COL_OK && len) {
            const u64 v = c.idx[r];
            w = q.tape[v];
            const u32 t = (u32)(w >> 56);
            if (t == '"') {
                wide = len > COL_SHORT;
                if (!wide) copy_bytes(arr_at(data, o, len), str_bytes(q, w, len), len, 0, 1);
            } else {
                u8 *dst = arr_at(data, o, len);
                if (t == 'l') (void)format_int(q.tape[v + 1], dst);
                else if (t == 'u') (void)format_uint(q.tape[v + 1], dst);
                else if (t == 'd') (void)format_float(q.tape[v + 1], dst);
                else {
                    const char *lit = t == 't' ? "true" : (t == 'f' ? "false" : "null");
                    for (u64 k = 0; k < len; k++) dst[k] = (u8)lit[k];
                }
            }
        }
    }
    wave_copy_strings(q, data, wide, o, len, w, lane);
}

// ---- list columns: the ARRAY at a path of every record, converted (sjhip_extract_path_list / sjhip_extract_path_list_strings) ----
// Arrow's large_list<T> / large_list<large_string>: u64 list offsets over the records, the elements end to end, and for strings
// u64 offsets over the elements with the bytes end to end.  The conversions are those of parsed_array.go:145-344 (Array.AsFloat /
// AsInteger / AsUint64 / AsString / AsStringCvt), which stop at the first element they cannot convert.  Three steps over the
// n = R + 1 records, like the string column:
//   measure   FindElement, Iter.Array, then the whole conversion check of the array: its status, its element count and (strings)
//             the bytes of its texts; entry n is 0
//   scan      exclusive prefixes of the n + 1 counts (and byte totals) in place: sums -> one-block scan (k_tw_scan_sums) -> apply
//   gather    the list offsets and statuses, the values (or the string offsets and bytes) of every OK record
// Values and float text are produced again in the gather rather than stashed (the trade of the string column, for its reason).
// An array runs from 0 to millions of elements, so one lane per record is not enough.  For the numeric kinds and AsString every
// acceptable element is two tape words: element k of the array opened at v is at v + 1 + 2k and there are (close - v - 1) / 2 of
// them, PROVIDED every element in front of it is acceptable.  A short array is handled by its record's lane; every longer array of
// the wave's 64 records by the whole wave in turn, 64 elements per step.  The first failing element is the lowest k of a step --
// one ballot -- whose tag word is not acceptable or whose value is out of range; every position below it is known to be a
// two-word element, the words behind it are never trusted: the walk stops at the first failing step.
// AsStringCvt mixes one-word (t f n) and two-word elements, so positions are not strided: these arrays are walked by their
// record's lane, whatever their length (a long array costs one lane's serial walk: DESIGN.md section 5b); strings longer than
// COL_SHORT bytes are copied by the whole wave for every variant.
static constexpr int LIST_STR = 4, LIST_CVT = 5;  // Array.AsString / AsStringCvt, behind SJHIP_COL_FLOAT / INT / UINT
static constexpr u64 LIST_SHORT = 16;             // elements a record's lane converts alone
struct QList {
    u64 *idx;                              // [n] tape index of the array's '['
    u64 *cnt;                              // [n + 1] elements of the record -> its list offset (entry n: the total)
    u64 *bytes;                            // [n + 1] strings: bytes of the record's texts -> their offset (entry n: the total); else null
    u8 *status;                            // [n]
    unsigned long long *tiles_c, *tiles_b; // [tiles] tile sums of cnt / bytes -> their exclusive prefixes
};
// Status of the two-word element at p for Array.AsFloat / AsInteger / AsUint64 (kind = SJHIP_COL_*) or AsString (LIST_STR), with
// its value bits / its byte length in *out.  Unlike Iter.Float / Int / Uint (element_to): null is a type error like any other tag
// (parsed_array.go:175,226,277), and AsUint64 rejects a float above math.MaxInt64 -- 2^63 as a float64 -- (:253) where Iter.Uint
// compares with 2^64; uint64(2^63) is 1 << 63.
__device__ __forceinline__ int list_elem(const QView &q, u64 p, int kind, u64 *out) {
    const u32 t = (u32)(q.tape[p] >> 56);
    *out = 0;
    if (kind == LIST_STR) {
        if (t != '"') return SJHIP_COL_TYPE;
        *out = q.tape[p + 1];
        return SJHIP_COL_OK;
    }
    if (t != 'l' && t != 'u' && t != 'd') return SJHIP_COL_TYPE;
    if (kind == SJHIP_COL_UINT && t == 'd') {
        const double d = __longlong_as_double((long long)q.tape[p + 1]);
        if (d > 9223372036854775808.0 || d < 0.0) return SJHIP_COL_RANGE;  // (-0.0 passes and converts to 0)
        *out = d >= 9223372036854775808.0 ? 0x8000000000000000ull : (u64)d;
        return SJHIP_COL_OK;
    }
    return element_to(q, p, kind, out);
}
// FindElement + Iter.Array on record r: SJHIP_COL_OK with the index of the '[' and of its ']', or the record's status
__device__ __forceinline__ int record_array(const QView &q, const QPath &pth, u32 r, u64 *v, u64 *close) {
    *v = record_find_path(q, pth, r);
    *close = 0;
    if (*v >= SJHIP_PATH_NOT_OBJECT) return path_status(*v);
    const u64 w = q.tape[*v];
    const u32 t = (u32)(w >> 56);
    if (t == 'n') return SJHIP_COL_NULL;
    if (t != '[') return SJHIP_COL_TYPE;  // "next item is not array"
    *close = (w & TW_PAYLOAD) - 1;
    return SJHIP_COL_OK;
}
// the strided conversion check of the array (v, close) by one lane (first = 0, step = 1) ...
__device__ __forceinline__ int lane_list_measure(const QView &q, u64 v, u64 close, int kind, u64 *cnt, u64 *bytes) {
    u64 sum = 0;
    for (u64 p = v + 1; p < close; p += 2) {
        u64 x;
        const int st = list_elem(q, p, kind, &x);
        if (st) return st;
        sum += x;
    }
    *cnt = (close - v - 1) / 2;
    *bytes = kind == LIST_STR ? sum : 0;
    return SJHIP_COL_OK;
}
// ... and by the whole wave, 64 elements per step (all arguments and the results wave-uniform)
__device__ __forceinline__ int wave_list_measure(const QView &q, u64 v, u64 close, int kind, int lane, u64 *cnt, u64 *bytes) {
    u64 sum = 0;
    for (u64 g = v + 1; g < close; g += 128) {
        const u64 p = g + 2 * (u64)lane;
        u64 x = 0;
        const int st = p < close ? list_elem(q, p, kind, &x) : SJHIP_COL_OK;
        const u64 bad = __ballot(st != SJHIP_COL_OK);
        if (bad) return __shfl(st, __ffsll((unsigned long long)bad) - 1, 64);  // the first failing element of the array
        sum += x;
    }
    *cnt = (close - v - 1) / 2;
    *bytes = kind == LIST_STR ? wave_sum(sum) : 0;
    return SJHIP_COL_OK;
}
__device__ __forceinline__ void list_measure_store(const QView &q, const QList &c, u32 r, u64 v, int st, u64 cnt, u64 bytes) {
    if (r < q_rows(q)) {
        c.idx[r] = v;
        c.cnt[r] = st == SJHIP_COL_OK ? cnt : 0;
        if (c.bytes) c.bytes[r] = st == SJHIP_COL_OK ? bytes : 0;
        c.status[r] = (u8)st;
    } else if (r == q_rows(q)) {
        c.cnt[r] = 0;
        if (c.bytes) c.bytes[r] = 0;
    }
}
__global__ __launch_bounds__(256) void k_q_list_measure(QView q, QPath pth, int kind, QList c) {
    const u32 r = blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    u64 v = 0, close = 0, cnt = 0, bytes = 0;
    int st = SJHIP_COL_NOT_FOUND;
    bool wide = false;
    if (r < q_rows(q)) {
        st = record_array(q, pth, r, &v, &close);
        if (st == SJHIP_COL_OK) {
            wide = close - v - 1 > 2 * LIST_SHORT;
            if (!wide) st = lane_list_measure(q, v, close, kind, &cnt, &bytes);
        }
    }
    // (by hand, not wave_each: with it the skewed FLOAT case of tools/list_column_time.py measured 2 % slower, here and in the gather)
    for (u64 todo = __ballot(wide); todo; todo &= todo - 1) {  // the wave's long arrays, one after another
        const int j = __ffsll((unsigned long long)todo) - 1;
        const u64 vj = (u64)__shfl((long long)v, j, 64), cj = (u64)__shfl((long long)close, j, 64);
        u64 n_j = 0, b_j = 0;
        const int st_j = wave_list_measure(q, vj, cj, kind, lane, &n_j, &b_j);
        if (lane == j) {
            st = st_j;
            cnt = n_j;
            bytes = b_j;
        }
    }
    list_measure_store(q, c, r, v, st, cnt, bytes);
}
// AsStringCvt: every element converted by StringCvt (element_text_len), one lane per record
__global__ __launch_bounds__(256) void k_q_list_measure_cvt(QView q, QPath pth, QList c) {
    const u32 r = blockIdx.x * 256 + threadIdx.x;
    u64 v = 0, close = 0, cnt = 0, bytes = 0;
    int st = SJHIP_COL_NOT_FOUND;
    if (r < q_rows(q)) {
        st = record_array(q, pth, r, &v, &close);
        for (u64 p = v + 1; st == SJHIP_COL_OK && p < close;) {
            u64 len;
            st = element_text_len(q, p, true, &len);  // (TYPE for { and [: nothing is skipped over)
            bytes += len;
            cnt++;
            p += two_word_tag(q.tape[p]) ? 2 : 1;
        }
    }
    list_measure_store(q, c, r, v, st, cnt, bytes);
}
__global__ __launch_bounds__(QT) void k_q_list_tile_sums(QList c, u32 m) {
    tile_sums(c.cnt, m, c.tiles_c);
    if (c.bytes) tile_sums(c.bytes, m, c.tiles_b);
}
__global__ __launch_bounds__(QT) void k_q_list_tile_apply(QList c, u32 m) {
    tile_apply(c.cnt, c.cnt, m, c.tiles_c);
    if (c.bytes) tile_apply(c.bytes, c.bytes, m, c.tiles_b);
}
// out_off[0 .. n] (the part's own list offsets, from 0), out_status[n], values: the elements.  A short array by its record's lane;
// a long one by the whole wave: lane l converts element g + l and stores it next to its neighbours' (consecutive 8-byte stores).
__global__ __launch_bounds__(256) void k_q_list_gather_num(QView q, QList c, int kind, u64 *out_off, u8 *out_status, Arr<u64> values) {
    const u32 r = blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    u64 o = 0, cnt = 0, v = 0;
    bool wide = false;
    if (r < q_rows(q)) {
        o = c.cnt[r];
        cnt = c.cnt[r + 1] - o;
        out_off[r] = o;
        out_status[r] = c.status[r];
        if (r + 1 == q_rows(q)) out_off[r + 1] = o + cnt;
        v = c.idx[r];
        wide = cnt > LIST_SHORT;  // (only an OK record has elements)
        if (!wide)
            for (u64 k = 0; k < cnt; k++) {
                u64 x;
                (void)list_elem(q, v + 1 + 2 * k, kind, &x);
                values[o + k] = x;
            }
    }
    // (by hand, not wave_each: with it the skewed FLOAT case of tools/list_column_time.py measured 2 % slower, here and in the measure)
    for (u64 todo = __ballot(wide); todo; todo &= todo - 1) {
        const int j = __ffsll((unsigned long long)todo) - 1;
        const u64 oj = (u64)__shfl((long long)o, j, 64), nj = (u64)__shfl((long long)cnt, j, 64), vj = (u64)__shfl((long long)v, j, 64);
        for (u64 k = (u64)lane; k < nj; k += 64) {
            u64 x;
            (void)list_elem(q, vj + 1 + 2 * k, kind, &x);
            values[oj + k] = x;
        }
    }
}
// Strings: soff[e] = where the text of element e starts in `data` (entry elems: the total).  Every lane walks the elements of
// its record's array (AsStringCvt: every array; AsString: the short ones), writes their offsets, the converted texts and the
// strings of up to COL_SHORT bytes; when it meets a longer string it waits, and the wave copies the waiting lanes' strings one
// after another, 64 bytes at a time, before the walks go on.  AsString's long arrays follow, each by the whole wave: 64 lengths
// per step, their prefix by a shuffle scan (consecutive 8-byte stores of the offsets), short strings by their lanes, long ones
// by the wave.
template <bool CVT>
__device__ __forceinline__ void list_gather_strings(const QView &q, const QList &c, u64 *out_off, u8 *out_status, Arr<u64> soff,
                                                    Arr<u8> data) {
    const u32 r = blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    u64 o = 0, cnt = 0, v = 0, at = 0;
    bool wide = false;
    if (r < q_rows(q)) {
        o = c.cnt[r];
        cnt = c.cnt[r + 1] - o;
        at = c.bytes[r];
        out_off[r] = o;
        out_status[r] = c.status[r];
        if (r + 1 == q_rows(q)) {
            out_off[r + 1] = o + cnt;
            soff[o + cnt] = c.bytes[r + 1];
        }
        v = c.idx[r];
        wide = !CVT && cnt > LIST_SHORT;
    }
    const u64 at0 = at;
    u64 p = v + 1, k = wide ? cnt : 0;
    for (;;) {
        u64 sw = 0, sl = 0, so = 0;
        bool pend = false;
        while (k < cnt && !pend) {
            const u64 w = q.tape[p];
            const u32 t = (u32)(w >> 56);
            u64 len = 0;
            soff[o + k] = at;
            if (t == '"') {
                len = q.tape[p + 1];
                if (len > COL_SHORT) {
                    pend = true;
                    sw = w;
                    sl = len;
                    so = at;
                } else if (len) copy_bytes(arr_at(data, at, len), str_bytes(q, w, len), len, 0, 1);
            } else if (CVT) {  // (AsString's elements are strings)
                (void)element_text_len(q, p, true, &len);
                u8 *dst = arr_at(data, at, len);
                if (t == 'l') (void)format_int(q.tape[p + 1], dst);
                else if (t == 'u') (void)format_uint(q.tape[p + 1], dst);
                else if (t == 'd') (void)format_float(q.tape[p + 1], dst);
                else {
                    const char *lit = t == 't' ? "true" : (t == 'f' ? "false" : "null");
                    for (u64 i = 0; i < len; i++) dst[i] = (u8)lit[i];
                }
            }
            at += len;
            k++;
            p += two_word_tag(w) ? 2 : 1;
        }
        if (!__ballot(pend)) break;
        wave_copy_strings(q, data, pend, so, sl, sw, lane);
    }
    if (CVT) return;
    wave_each(wide, [&](int j) {  // AsString: the wave's long arrays, one after another
        const u64 oj = wave_bcast(o, j), nj = wave_bcast(cnt, j), vj = wave_bcast(v, j);
        u64 base = wave_bcast(at0, j);
        for (u64 g = 0; g < nj; g += 64) {
            const u64 e = g + (u64)lane;
            const bool in = e < nj;
            const u64 w = in ? q.tape[vj + 1 + 2 * e] : 0, len = in ? q.tape[vj + 2 + 2 * e] : 0;
            const u64 incl = wave_incl_sum(len, lane), mine = base + incl - len;
            if (in) {
                soff[oj + e] = mine;
                if (len && len <= COL_SHORT) copy_bytes(arr_at(data, mine, len), str_bytes(q, w, len), len, 0, 1);
            }
            wave_copy_strings(q, data, len > COL_SHORT, mine, len, w, lane);
            base += wave_bcast(incl, 63);
        }
    });
}
__global__ __launch_bounds__(256) void k_q_list_gather_str(QView q, QList c, u64 *out_off, u8 *out_status, Arr<u64> soff, Arr<u8> data) {
    list_gather_strings<false>(q, c, out_off, out_status, soff, data);
}
__global__ __launch_bounds__(256) void k_q_list_gather_cvt(QView q, QList c, u64 *out_off, u8 *out_status, Arr<u64> soff, Arr<u8> data) {
    list_gather_strings<true>(q, c, out_off, out_status, soff, data);
}

// ---- tables: columns at SEVERAL paths from one walk of every record (sjhip_extract_table) -----------------------------------------
// One lane per record runs table_walk (sj_tablewalk.h) over the plan of the table (sj_table.h); what it resolves goes straight
// through the conversions of the single columns -- element_to into the column's values and statuses in the table arena,
// element_text_len into the idx / off / status of the column's QCol -- so the string columns go on through k_q_col_tile_sums,
// k_tw_scan_sums, k_q_col_tile_apply and k_q_col_gather as they are (the gather reads idx and does not walk).  Every array is
// a column of its own: the 64 lanes of a wave store next to each other.  The resume stack of the walk is LDS: 2 x 16 u32 per
// lane, lane after lane in every row (no bank conflicts), 32 KiB per block of 256.
struct QTable {
    TablePlan pl;
    Arr<u8> out;   // the table arena of the part: values and statuses of the numeric / bool columns
    Arr<u8> work;  // the work arrays of the string columns (their QCol)
    // byte offsets, column by column: numeric / bool: values and status in `out`; strings: idx, off and status in `work`
    u64 a_off[TABLE_MAX_COLS], b_off[TABLE_MAX_COLS], st_off[TABLE_MAX_COLS];
};
static_assert(sizeof(QView) + sizeof(QTable) <= 4096, "k_q_table_walk: the view and the plan travel as kernel arguments (4 KiB)");
struct TableView {
    const QView &q;
    __device__ __forceinline__ u64 word(u64 i) const { return q.tape[i]; }
    __device__ __forceinline__ bool key_equals(u64 kw, u64 kl, u32 key_b, u32 key_n) const { return str_equals(q, kw, kl, q.key + key_b, key_n); }
};
struct TableSink {
    const QView &q;
    const QTable &t;
    u32 r;
    __device__ __forceinline__ void operator()(u32 c, u64 v) const {
        const int kind = t.pl.kind[c];
        u64 x = 0;
        if (kind <= SJHIP_COL_BOOL) {
            const int st = v < SJHIP_PATH_NOT_OBJECT ? element_to(q, v, kind, &x) : path_status(v);
            if (kind == SJHIP_COL_BOOL) *arr_at(t.out, t.a_off[c] + r, 1) = (u8)x;
            else *(u64 *)arr_at(t.out, t.a_off[c] + 8ull * r, 8) = x;
            *arr_at(t.out, t.st_off[c] + r, 1) = (u8)st;
        } else {
            const int st = v < SJHIP_PATH_NOT_OBJECT ? element_text_len(q, v, kind == SJHIP_COL_STRING_CVT, &x) : path_status(v);
            *(u64 *)arr_at(t.work, t.a_off[c] + 8ull * r, 8) = v;
            *(u64 *)arr_at(t.work, t.b_off[c] + 8ull * r, 8) = x;
            *arr_at(t.work, t.st_off[c] + r, 1) = (u8)st;
        }
    }
};
__global__ __launch_bounds__(256) void k_q_table_walk(QView q, QTable t) {
    __shared__ u32 s_stack[TABLE_STACK_WORDS * 256];
    const u32 r = blockIdx.x * 256 + threadIdx.x;
    if (r >= q_rows(q)) {
        if (r == q_rows(q))  // entry n of every string column's lengths, as k_q_col_len leaves it
            for (u32 c = 0; c < t.pl.n_cols; c++)
                if (t.pl.kind[c] > SJHIP_COL_BOOL) *(u64 *)arr_at(t.work, t.b_off[c] + 8ull * r, 8) = 0;
        return;
    }
    const TableView view = {q};
    TableSink sink = {q, t, r};
    table_walk(view, t.pl, row_value(q, r), s_stack + threadIdx.x, 256u, sink);
}


// ---- row selection: the elements of the ARRAY at a path of every record become the rows (sjhip_select_rows) -------------------------
// The reference's FindElement(path...) -> Iter.Array() -> Array.Iter() / Advance over the elements, for every record at once.  An
// array runs from 0 to millions of elements and its elements are containers of any size, so the row starts are found by passes
// over the TAPE, not by a walk of the array:
//   k_q_rows_records   one lane per record: record_array -- the index of the target '[' and of its ']' (0, 0: no rows), the status
//   k_q_rows_tile<0>   per 2048-word tile: the sum of the depth deltas of its tag words (+1 for { [, -1 for } ])
//   k_tw_scan_sums     the depth in front of every tile (the signed deltas wrap correctly in the unsigned sums)
//   k_q_rows_tile<1>   per tile: its row starts, counted;  k_tw_scan_sums: the row number of the first one, and the total
//   k_q_rows_tile<2>   the row starts again, written to row_index at their row numbers (the gather: d_rows has that size now)
//   k_q_rows_offsets   one lane per record: row_offsets[r] = the rows in front of the record (a lower bound in row_index)
// A word i is a row start iff it is a tag word (the anchor rule of sj_tapewalk.h), its tag is none of } ] r, its depth -- counted
// from 0 at its record's root value -- is n_keys + 1, and it lies strictly inside the target array of its record.  FindElement
// descends objects only, so the array at a path of n keys sits at depth exactly n and a word at depth n + 1 inside its range is a
// direct element, whatever lies inside the elements.  Records are balanced and the roots carry no depth, so the depth is one
// prefix sum over the whole tape.  A word learns its record by a search of nl_off -- once per lane, then at most one step per
// word -- and reads the record's range from what the record lanes stored: no bitmap to clear and set, no running maximum to
// scan.  No lane's work grows with the length of an array.
// The tiles find the anchor of the tag / raw classification among the 64 words in front of them (tw_local_anchor); a tile that
// cannot raises totals[3], and then -- decided on the device, nothing waits for the host -- k_q_rows_last / k_q_rows_scan_last
// compute the global anchors, the depth pass runs again with them and the later passes use them.  Without the flag those three
// launches end at once.
struct QRows {
    u64 *open, *close;            // [n] merged tape index of the record's target '[' and of its ']' (0, 0: the record has no rows)
    u8 *status;                   // [n]
    unsigned long long *depth;    // [tiles] sum of the depth deltas of the tile -> the depth in front of it
    unsigned long long *cnt;      // [tiles] row starts of the tile -> the row number of its first
    long long *tile_last;         // [tiles] the global anchors (only when a tile asked for them)
    unsigned long long *totals;   // [1] the rows; [3] != 0: a tile found no anchor among the 64 words in front of it
    u32 depth_want;               // n_keys + 1
};
// FindElement + Iter.Array on row r (record r without a selection), the path may be empty: the row's own value is then the array
__device__ __forceinline__ int row_array(const QView &q, const QPath &pth, u32 r, u64 *v, u64 *close) {
    if (pth.n) return record_array(q, pth, r, v, close);
    *v = row_value(q, r);
    const u64 w = q.tape[*v];
    const u32 t = (u32)(w >> 56);
    *close = (w & TW_PAYLOAD) - 1;
    return t == 'n' ? SJHIP_COL_NULL : (t != '[' ? SJHIP_COL_TYPE : SJHIP_COL_OK);
}
__global__ __launch_bounds__(256) void k_q_rows_records(QView q, QPath pth, QRows o) {
    const u32 r = blockIdx.x * 256 + threadIdx.x;
    if (r > q.R) return;
    u64 v = 0, close = 0;  // (an empty path: Iter.Array on the root value itself)
    const int st = row_array(q, pth, r, &v, &close);
    o.open[r] = st == SJHIP_COL_OK ? v : 0;
    o.close[r] = st == SJHIP_COL_OK ? close : 0;
    o.status[r] = (u8)st;
}
__global__ __launch_bounds__(TW_THREADS) void k_q_rows_last(QView q, QRows o) {
    __shared__ long long s_w[TW_THREADS / 64];
    if (o.totals[3] == 0) return;
    tw_tile_last(arr_raw(q.tape) + q.tape_base, q.tape_len - q.tape_base, o.tile_last, s_w);
}
__global__ __launch_bounds__(1024) void k_q_rows_scan_last(QRows o, u32 tiles) {
    __shared__ long long s_w[16];
    if (o.totals[3] == 0) return;
    block1024_scan_array<true>(o.tile_last, tiles, s_w, (int)threadIdx.x);
}
// What both tile walks -- the row selection's and the unnest's -- start from: the thread's TW_ITEMS words of the tile classified by
// the anchor rule.  tags: the tag words whose tag may start a row (none of } ] r); opens / closes: the brackets among the tag words.
// !ok (block-uniform, and only without the global anchors): no anchor among the 64 words in front of the tile, nothing can be
// classified.  Indices are local to the part's tape here.
struct TileTags { u32 tags, opens, closes; bool ok; };
__device__ __forceinline__ TileTags tile_classify(const QView &q, const QRows &o, bool global, long long *s_l, long long *s_carry) {
    const int tid = threadIdx.x;
    const u64 n = q.tape_len - q.tape_base;
    const u64 base = (u64)blockIdx.x * TW_TILE + (u64)tid * TW_ITEMS;
    u64 w[TW_ITEMS];
#pragma unroll
    for (int k = 0; k < TW_ITEMS; k++) w[k] = base + k < n ? q.tape[q.tape_base + base + k] : 0;
    long long last = -1;
#pragma unroll
    for (int k = 0; k < TW_ITEMS; k++)
        if (base + k < n && !two_word_tag(w[k])) last = (long long)(base + k);
    long long anchor = block_excl_max(last, s_l, tid);  // last anchor in front of this thread's words, inside the tile
    const long long carry = global ? o.tile_last[blockIdx.x]
                                   : tw_local_anchor(arr_raw(q.tape) + q.tape_base, (u64)blockIdx.x * TW_TILE, tid, s_carry);
    if (carry == -2) return {0u, 0u, 0u, false};
    anchor = anchor > carry ? anchor : carry;
    u32 tags = 0, opens = 0, closes = 0;
#pragma unroll
    for (int k = 0; k < TW_ITEMS; k++) {
        const u64 i = base + k;
        if (i >= n) continue;
        const bool raw = anchor >= 0 && ((((long long)i - anchor - 1) & 1) != 0);
        if (!two_word_tag(w[k])) anchor = (long long)i;
        if (raw) continue;
        const u32 t = (u32)(w[k] >> 56);
        if (t == '{' || t == '[') opens |= 1u << k;
        else if (t == '}' || t == ']') closes |= 1u << k;
        if (t != '}' && t != ']' && t != 'r') tags |= 1u << k;
    }
    return {tags, opens, closes, true};
}
// The row starts among the thread's words, as a mask: the words of `tags` whose depth is `want` and that inside(k) accepts --
// called for those words only, in ascending k.  depth: in front of the thread's first word.
template <typename F>
__device__ __forceinline__ u32 tile_starts(u32 tags, u32 opens, u32 closes, int depth, int want, F inside) {
    u32 starts = 0;
#pragma unroll
    for (int k = 0; k < TW_ITEMS; k++) {
        const u32 bit = 1u << k;
        if ((tags & bit) && depth == want && inside(k)) starts |= bit;
        depth += (int)((opens >> k) & 1u) - (int)((closes >> k) & 1u);
    }
    return starts;
}
// MODE 0: the depth sums (`again`: the second run, with the global anchors, if a tile of the first one asked for them);
// 1: the row starts counted; 2: written.  Indices are local to the part's tape here; what is stored and compared is merged.
template <int MODE>
__global__ __launch_bounds__(TW_THREADS) void k_q_rows_tile(QView q, QRows o, u32 again, Arr<u64> row_index) {
    __shared__ long long s_l[TW_THREADS / 64];
    __shared__ unsigned long long s_s[TW_THREADS / 64];
    __shared__ long long s_carry;
    const int tid = threadIdx.x;
    const bool global = MODE == 0 ? again != 0 : o.totals[3] != 0;  // (the first depth pass raises the flag: it must not read it)
    if (MODE == 0 && again && o.totals[3] == 0) return;
    const u64 base = (u64)blockIdx.x * TW_TILE + (u64)tid * TW_ITEMS;
    const TileTags c = tile_classify(q, o, global, s_l, &s_carry);
    const u32 tags = c.tags, opens = c.opens, closes = c.closes;
    if (!c.ok) {  // (only the first depth pass)
        if (tid == 0) {
            atomicOr(&o.totals[3], 1ull);
            o.depth[blockIdx.x] = 0;
        }
        return;
    }
    const int delta = __popc(opens) - __popc(closes);
    unsigned long long tot = 0;
    const unsigned long long ex = block_excl_sum((unsigned long long)(long long)delta, s_s, tid, &tot);
    if (MODE == 0) {
        if (tid == 0) o.depth[blockIdx.x] = tot;
        return;
    }
    u32 r = NONE32;
    const u32 starts = tile_starts(tags, opens, closes, (int)(u32)(o.depth[blockIdx.x] + ex), (int)o.depth_want, [&](int k) {
        const u64 il = base + k;  // (a word inside a record: never a root)
        if (r == NONE32) {        // the record of the word: the first whose closing root lies behind it
            u32 lo = 0, hi = q.R;
            while (lo < hi) {
                const u32 mid = lo + (hi - lo) / 2;
                if (q.nl_off[mid] < il) lo = mid + 1;
                else hi = mid;
            }
            r = lo;
        } else {
            while (r < q.R && q.nl_off[r] < il) r++;  // (a record is three words or more: two steps at the most per word)
        }
        const u64 i = q.tape_base + il;
        return o.open[r] < i && i < o.close[r];
    });
    unsigned long long at = block_excl_sum((unsigned long long)__popc(starts), s_s, tid, &tot);
    if (MODE == 1) {
        if (tid == 0) o.cnt[blockIdx.x] = tot;
        return;
    }
    at += o.cnt[blockIdx.x];
#pragma unroll
    for (int k = 0; k < TW_ITEMS; k++)
        if (starts & (1u << k)) row_index[at++] = q.tape_base + base + k;
}
// the rows in front of tape index `first`: a lower bound in the row index (the row starts are in document order)
__device__ __forceinline__ u64 rows_below(const Arr<const u64> &row_index, u64 rows, u64 first) {
    u64 lo = 0, hi = rows;
    while (lo < hi) {
        const u64 mid = lo + (hi - lo) / 2;
        if (row_index[mid] < first) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
// row_offsets[r] = the rows in front of record r: the row starts below its opening root (they are in document order)
__global__ __launch_bounds__(256) void k_q_rows_offsets(QView q, QRows o, Arr<const u64> row_index, u64 rows, u64 *out_off, u8 *out_status) {
    const u32 r = blockIdx.x * 256 + threadIdx.x;
    if (r > q.R) return;
    out_off[r] = rows_below(row_index, rows, rec_open(q, r));
    out_status[r] = o.status[r];
    if (r == q.R) out_off[r + 1] = rows;
}

// ---- unnest rows: the array at a path of every ROW becomes the rows (sjhip_unnest_rows) --------------------------------------------
// The row selection one level further down: FindElement + Iter.Array on the value of every row in force -- the parents; without a
// selection the root values of the records -- and the direct elements of those arrays, in document order, are the new rows.
//   k_q_unnest_parents  one lane per parent row: row_array on the view with rows -> the target '[', its ']' and the status
//   the depth prefix    the row selection's own passes (k_q_rows_tile<0>, k_q_rows_last, k_q_rows_scan_last, k_tw_scan_sums)
//   k_q_unnest_tile<1>  per tile: its new row starts, counted;  k_tw_scan_sums: the row number of the first one, and the total
//   k_q_unnest_tile<2>  the row starts again, written at their row numbers with the number of their parent beside them
//   k_q_rows_offsets    one lane per record: the new rows in front of it, its status byte handed on
//   k_q_unnest_offsets  one lane per parent: parent_offsets[p] = the new rows in front of its value, its status byte
// A word is a new row start iff it is a tag word, its tag is none of } ] r, its depth is that of the parents + n_keys + 1 (all rows
// of a selection lie at one depth below their record's root, which the selection carries: ResultState::Rows::depth) and it lies
// strictly inside the target range of its parent.  A word learns its parent -- the last old row that starts below it -- by one
// search of the old row index per lane, then by stepping: rows are disjoint, in document order and at least one word long, so
// there is at most one step per word.  No lane's work grows with the length of an array or the size of an element.
struct QUnnest {
    QRows t;                      // the tile passes: depth, cnt, tile_last, totals, depth_want (open, close, status: unused)
    Arr<u64> open, close;         // [n] merged tape index of the parent's target '[' and of its ']' (0, 0: the parent has no rows)
    Arr<u8> status;               // [n]
};
__global__ __launch_bounds__(256) void k_q_unnest_parents(QView q, QPath pth, QUnnest u) {
    const u32 p = blockIdx.x * 256 + threadIdx.x;
    if (p >= q_rows(q)) return;
    u64 v = 0, close = 0;
    const int st = row_array(q, pth, p, &v, &close);
    u.open[p] = st == SJHIP_COL_OK ? v : 0;
    u.close[p] = st == SJHIP_COL_OK ? close : 0;
    u.status[p] = (u8)st;
}
// MODE 1: the new row starts counted; 2: written, each with its parent (the depth sums are the row selection's MODE 0).
// MEMBERS (sjhip_unnest_members, below): the parents' targets are objects, the starts inside them alternate key, value, and the
// rows are the values -- the starts of odd rank; the tile counts carry starts, two to a row.
template <int MODE, bool MEMBERS>
__device__ __forceinline__ void unnest_tile(const QView &q, const QUnnest &u, Arr<u64> row_index, Arr<u64> parent) {
    static_assert(MODE == 1 || MODE == 2, "count or write");
    // (the LDS below belongs to the kernel this is inlined into: each of the four instantiations gets its own copy)
    __shared__ long long s_l[TW_THREADS / 64];
    __shared__ unsigned long long s_s[TW_THREADS / 64];
    __shared__ long long s_carry;
    const int tid = threadIdx.x;
    const QRows &o = u.t;
    const u64 base = (u64)blockIdx.x * TW_TILE + (u64)tid * TW_ITEMS;
    const TileTags c = tile_classify(q, o, o.totals[3] != 0, s_l, &s_carry);
    const u32 tags = c.tags, opens = c.opens, closes = c.closes;
    if (!c.ok) return;  // (the depth pass settled it: never)
    unsigned long long tot = 0;
    const unsigned long long ex = block_excl_sum((unsigned long long)(long long)(__popc(opens) - __popc(closes)), s_s, tid, &tot);
    const u32 n = q_rows(q);
    u32 below = NONE32;    // the parents that start below the word
    u32 par[TW_ITEMS];     // (MODE 2) the parent of the start at word k
    const u32 starts = tile_starts(tags, opens, closes, (int)(u32)(o.depth[blockIdx.x] + ex), (int)o.depth_want, [&](int k) {
        const u64 i = q.tape_base + base + k;
        if (below == NONE32) {
            u32 lo = 0, hi = n;
            while (lo < hi) {
                const u32 mid = lo + (hi - lo) / 2;
                if (row_value(q, mid) < i) lo = mid + 1;
                else hi = mid;
            }
            below = lo;
        } else {
            while (below < n && row_value(q, below) < i) below++;
        }
        if (below == 0) return false;
        if (MODE == 2) par[k] = below - 1u;
        return u.open[below - 1u] < i && i < u.close[below - 1u];
    });
    unsigned long long at = block_excl_sum((unsigned long long)__popc(starts), s_s, tid, &tot);
    if (MODE == 1) {
        if (tid == 0) o.cnt[blockIdx.x] = tot;
        return;
    }
    at += o.cnt[blockIdx.x];
#pragma unroll
    for (int k = 0; k < TW_ITEMS; k++)
        if (starts & (1u << k)) {
            if (!MEMBERS) {
                row_index[at] = q.tape_base + base + k;
                parent[at] = par[k];
            } else if (at & 1u) {  // (an even rank: the member's key)
                row_index[at >> 1] = q.tape_base + base + k;
                parent[at >> 1] = par[k];
            }
            at++;
        }
}
template <int MODE>
__global__ __launch_bounds__(TW_THREADS) void k_q_unnest_tile(QView q, QUnnest u, Arr<u64> row_index, Arr<u64> parent) {
    unnest_tile<MODE, false>(q, u, row_index, parent);
}
// parent_offsets[p] = the new rows in front of parent p: the new row starts below its value (entry n: all of them)
__global__ __launch_bounds__(256) void k_q_unnest_offsets(QView q, QUnnest u, Arr<const u64> row_index, u64 rows, Arr<u64> out_off, Arr<u8> out_status) {
    const u32 p = blockIdx.x * 256 + threadIdx.x, n = q_rows(q);
    if (p > n) return;
    out_off[p] = p < n ? rows_below(row_index, rows, row_value(q, p)) : rows;
    if (p < n) out_status[p] = u.status[p];
}

// ---- member rows: the members of the OBJECT at a path of every row become the rows (sjhip_unnest_members) ---------------------------
// The unnest with Iter.Object in the place of Iter.Array: FindElement + Iter.Object on the value of every parent, and the VALUES of
// the direct members of those objects, in document order, are the new rows (Object.ForEach / NextElementBytes visit them so:
// duplicate names each give a row).  The passes are the unnest's, with two kernels of their own:
//   k_q_members_parents  one lane per parent row: row_object -> the target '{', its '}' and the status, into the unnest's arrays
//   k_q_members_tile<1>  per tile: the STARTS inside the targets, counted -- keys and values together;  k_tw_scan_sums: the rank
//                        of the tile's first start, and the total (the host halves it: the rows)
//   k_q_members_tile<2>  the starts again; the one of rank 2j + 1 is the value of member j: row_index[j], parent[j]
// A start is what the unnest calls one: a tag word at the parents' depth + n_keys + 1 strictly inside the target of its parent.
// Inside an object those are the key and the value of every direct member, alternating: a key is a string, two words whose second
// is raw by the anchor rule, and a value is one start whatever lies inside it.  Every OK parent contributes an even number of them,
// the parents are disjoint and in document order, so the rank of a start among all starts of the PART is even for a key and odd
// for a value -- the prefix the count pass computes anyway; a tile that holds an odd number of starts hands the parity on in its
// prefix.  No object is walked, and no lane's work grows with the members of an object.  The name of a row is not stored: it is
// the string whose tag word lies two words in front of the row's value (k_q_names_len, k_q_names_mark), which holds for every
// selection narrowed from this one as well.
// FindElement + Iter.Object on row r (record r without a selection); an empty path: the row's own value is the object
__device__ __forceinline__ int row_object(const QView &q, const QPath &pth, u32 r, u64 *v, u64 *close) {
    *v = pth.n ? record_find_path(q, pth, r) : row_value(q, r);
    *close = 0;
    if (*v >= SJHIP_PATH_NOT_OBJECT) return path_status(*v);
    const u64 w = q.tape[*v];
    const u32 t = (u32)(w >> 56);
    if (t == 'n') return SJHIP_COL_NULL;
    if (t != '{') return SJHIP_COL_TYPE;  // "next item is not object"
    *close = (w & TW_PAYLOAD) - 1;
    return SJHIP_COL_OK;
}
__global__ __launch_bounds__(256) void k_q_members_parents(QView q, QPath pth, QUnnest u) {
    const u32 p = blockIdx.x * 256 + threadIdx.x;
    if (p >= q_rows(q)) return;
    u64 v = 0, close = 0;
    const int st = row_object(q, pth, p, &v, &close);
    u.open[p] = st == SJHIP_COL_OK ? v : 0;
    u.close[p] = st == SJHIP_COL_OK ? close : 0;
    u.status[p] = (u8)st;
}
template <int MODE>
__global__ __launch_bounds__(TW_THREADS) void k_q_members_tile(QView q, QUnnest u, Arr<u64> row_index, Arr<u64> parent) {
    unnest_tile<MODE, true>(q, u, row_index, parent);
}

// ---- row schema: the distinct member names of the rows, counted per value type (sjhip_row_schema) -----------------------------------
// "Which names do these rows have, how often, and with values of which types": FindElement + Iter.Object on every row in force, as
// sjhip_unnest_members evaluates it, and every direct member of those objects counted under (its unescaped name, the Type of its
// value).  Names are numbered by first occurrence in document order, so the dictionary, first_row and the counts are decided by the
// input alone.  The selection and every other product are read, never written: the member walk runs into the work arenas.
//   the member walk     k_q_members_parents, the depth prefix, k_q_members_tile<1>, the scan, k_q_members_tile<2> -- launched as
//                       sjhip_unnest_members launches them -- leave the value index of every member (idx[j], document order) and the
//                       number of its parent row (parent[j])
//   k_q_schema_status   the parents' status bytes counted: six ballots per 64 parents, four such steps per wave, then ONE atomic
//                       instruction per wave -- lane s adds the count of status s
//   k_q_schema_keys     one lane per member: the name is the string two words in front of the value (k_q_names_len); its hash
//                       (sj_group.h, over the unescaped bytes wherever they lie: str_bytes) and the type class of the value's tag
//   k_q_schema_insert   the dictionary: k_q_group_insert's open-addressing table of MEMBER numbers behind a wave-level election, below
//   k_q_schema_first    member j is the first of its name iff table[slot[j]] == j -> flag, and the length of its name; exclusive
//                       scans (k_q_schema_tile_sums, k_tw_scan_sums, k_q_schema_tile_apply) number the names and place their bytes;
//                       the totals are the names and the dictionary's bytes -- the one value of the second half the host waits for
//   k_q_schema_emit     every member: the sort key code * 8 + class; the first members: their name's offset, bytes (a short name by
//                       the lane, a long one by the wave) and first_row = the parent row
//   the sort            sj_sort.h, stable, over only the digits names * 8 has
//   k_q_schema_bounds   in the sorted keys a run of one key begins where the key in front differs and ends where the next one does
//   k_q_schema_counts   counts[key] = end - begin (0, 0 for a key that does not occur) -- no contended atomics anywhere
// THE ELECTION.  A schema call brings tens of members per row to a handful of names: on parking-citations a million rows are
// twenty million members on about twenty slots.  In k_q_group_insert every lane probes for itself, so the 64 lanes of a wave issue
// 64 atomic loads that land on a few L2 lines -- the channel serialises them -- and then compare their bytes with the occupant's.
// Here the wave first settles what it can inside itself, in at most SCHEMA_ELECT_ROUNDS rounds: the lowest pending lane is the
// leader (one ballot, one find-first-set); its hash, name length and string word are broadcast (three shuffles); every pending lane
// whose hash and length equal the leader's compares its name's bytes with the leader's -- all of them read the same addresses, one
// request --; the leader alone probes the table, exactly as k_q_group_insert probes it, and the slot it ended in is broadcast; the
// lanes whose bytes matched take that slot and retire.  The lanes still pending after the rounds probe for themselves.
// Why this is the same dictionary: (1) a lane takes the leader's slot only after comparing the bytes -- equal hashes with different
// bytes stay pending, nothing merges; (2) a pending lane either matches the leader, or stays pending and reaches its own probe, so
// nothing is lost; (3) a name ends in the first slot of its probe sequence that did not hold a different name whoever probes for it
// (the argument of k_q_group_insert), so the leader's slot IS the slot of every lane with its name; (4) member numbers grow with
// the lane, so a leader is the smallest member of its name in its wave; the smallest member of a name in the whole input is
// therefore never retired by another lane -- it probes, as a leader or for itself -- and atomicMin leaves it in the slot.
// SCHEMA_ELECT_ROUNDS is measured, not reasoned (tools/schema_time.py --exp, profiles/r37_schema_time.txt; DESIGN.md, Row schema): against
// no election, 2 rounds take 4 % off the call on parking-citations (19 names cycling through every wave) and 25 % on the users of
// twitter, and cost nothing on 2^20 distinct names; 4 rounds are the best on twitter but 5 % SLOWER than none on parking, 8 and 24
// lose everywhere -- a round serialises a probe behind a broadcast, and a wave that holds more distinct names than rounds pays for
// the rounds and still sends most of its lanes to the table.
static constexpr u32 SCHEMA_ELECT_ROUNDS = 2;
struct QSchema {
    u32 n, mask;          // the members; the table's capacity - 1
    Arr<u64> idx;         // [n] tape index of the member's value, in document order
    Arr<u64> parent;      // [n] the row the member belongs to
    Arr<u64> hash;        // [n] of the name's bytes
    Arr<u8> cls;          // [n] SJHIP_TYPE_* - 1 of the value
    Arr<u32> slot;        // [n] the slot the member's name ended in
    Arr<u32> table;       // [mask + 1] member numbers (empty: GROUP_NONE)
    Arr<u32> flag;        // [n + 1] 1 at the first member of a name -> exclusive prefix: the name's number
    Arr<u64> len;         // [n + 1] bytes of a first member's name -> their offset in the dictionary
    unsigned long long *tiles_f, *tiles_l;  // [tiles] each
};
struct SchemaOut {
    Arr<u64> name_off;   // [names + 1]
    Arr<u64> first_row;  // [names]
    Arr<u8> name_data;   // [name bytes]
};
// the reference's Type of a value, from its tape tag (TagToType, parsed_json.go), minus one
__device__ __forceinline__ u32 schema_class(u64 w) {
    switch ((u32)(w >> 56)) {
        case '"': return SJHIP_TYPE_STRING - 1;
        case 'l': return SJHIP_TYPE_INT - 1;
        case 'u': return SJHIP_TYPE_UINT - 1;
        case 'd': return SJHIP_TYPE_FLOAT - 1;
        case 't':
        case 'f': return SJHIP_TYPE_BOOL - 1;
        case '{': return SJHIP_TYPE_OBJECT - 1;
        case '[': return SJHIP_TYPE_ARRAY - 1;
        default: return SJHIP_TYPE_NULL - 1;  // 'n' (a member's value has no other tag)
    }
}
static constexpr int SCHEMA_STATUS_STEPS = 4;  // 64-parent steps per wave of k_q_schema_status
__global__ __launch_bounds__(256) void k_q_schema_status(QUnnest u, u32 n, Arr<unsigned long long> hist) {
    const u32 lane = threadIdx.x & 63u;
    const u32 base = (blockIdx.x * 4u + (threadIdx.x >> 6)) * (64u * SCHEMA_STATUS_STEPS);
    unsigned long long mine = 0;
    for (int k = 0; k < SCHEMA_STATUS_STEPS; k++) {
        const u32 p = base + (u32)k * 64u + lane;
        const u32 st = p < n ? (u32)u.status[p] : NONE32;
#pragma unroll
        for (u32 s = 0; s <= (u32)SJHIP_COL_RANGE; s++) {
            const u64 b = __ballot(st == s);
            if (lane == s) mine += (unsigned long long)__popcll(b);
        }
    }
    if (lane <= (u32)SJHIP_COL_RANGE && mine) atomicAdd(&hist[lane], mine);
}
__global__ __launch_bounds__(256) void k_q_schema_keys(QView q, QSchema s) {
    const u32 j = blockIdx.x * 256 + threadIdx.x;
    if (j >= s.n) return;
    const u64 v = s.idx[j];
    const u64 len = q.tape[v - 1];
    s.hash[j] = group_hash_bytes(str_bytes(q, q.tape[v - 2], len), len);
    s.cls[j] = (u8)schema_class(q.tape[v]);
}
// k_q_group_insert's probe for member j, whose name is the `len` bytes of the string word kw with hash h: the slot it ended in
__device__ __forceinline__ u32 schema_probe(const QView &q, const QSchema &s, u32 j, u64 h, u64 kw, u64 len) {
    u32 at = (u32)h & s.mask;
    for (u32 step = 0; step <= s.mask; step++, at = (at + 1u) & s.mask) {
        u32 *const cell = &s.table[at];
        u32 cur = __hip_atomic_load(cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == GROUP_NONE) {
            cur = atomicCAS(cell, GROUP_NONE, j);
            if (cur == GROUP_NONE) break;  // claimed
        }
        if (cur == j) break;
        if (s.hash[cur] != h) continue;
        const u64 vc = s.idx[cur];
        if (q.tape[vc - 1] != len || !group_bytes_equal(str_bytes(q, kw, len), str_bytes(q, q.tape[vc - 2], len), len)) continue;
        if (cur > j) (void)atomicMin(cell, j);
        break;
    }
    return at;
}
// E: the election's rounds.  The product instantiates SCHEMA_ELECT_ROUNDS alone; E = 0 is k_q_group_insert's protocol on members, with
// no election code in it (SJ_EXP builds instantiate it, and a few other counts, for the A/B of tools/schema_time.py).
template <u32 E>
__global__ __launch_bounds__(256) void k_q_schema_insert(QView q, QSchema s) {
    const u32 j = blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bool pending = j < s.n;
    u64 h = 0, kw = 0, len = 0;
    if (pending) {
        const u64 v = s.idx[j];
        kw = q.tape[v - 2];
        len = q.tape[v - 1];
        h = s.hash[j];
    }
    u32 mine = 0;
#pragma unroll 1
    for (u32 round = 0; round < E; round++) {
        const u64 todo = __ballot(pending);
        if (!todo) break;  // (wave-uniform)
        const int leader = __ffsll((unsigned long long)todo) - 1;
        const u64 h_l = wave_bcast(h, leader), len_l = wave_bcast(len, leader), kw_l = wave_bcast(kw, leader);
        const bool same = pending && h == h_l && len == len_l &&
                          (lane == leader || group_bytes_equal(str_bytes(q, kw, len), str_bytes(q, kw_l, len), len));
        u32 at = 0;
        if (lane == leader) at = schema_probe(q, s, j, h, kw, len);
        at = wave_bcast(at, leader);
        if (same) {
            mine = at;
            pending = false;
        }
    }
    if (pending) mine = schema_probe(q, s, j, h, kw, len);
    if (j < s.n) s.slot[j] = mine;
}
// (one lane per entry of the n + 1: entry n is 0, the scans leave the totals there)
__global__ __launch_bounds__(256) void k_q_schema_first(QView q, QSchema s) {
    const u32 j = blockIdx.x * 256 + threadIdx.x;
    if (j > s.n) return;
    const bool first = j < s.n && s.table[s.slot[j]] == j;
    s.flag[j] = first ? 1u : 0u;
    s.len[j] = first ? q.tape[s.idx[j] - 1] : 0ull;
}
__global__ __launch_bounds__(QT) void k_q_schema_tile_sums(QSchema s, u32 m) {
    tile_sums(arr_at(s.flag, 0, m), m, s.tiles_f);
    tile_sums(arr_at(s.len, 0, m), m, s.tiles_l);
}
__global__ __launch_bounds__(QT) void k_q_schema_tile_apply(QSchema s, u32 m) {
    u32 *const flag = arr_at(s.flag, 0, m);
    u64 *const len = arr_at(s.len, 0, m);
    tile_apply(flag, flag, m, s.tiles_f);
    tile_apply(len, len, m, s.tiles_l);
}
__global__ __launch_bounds__(256) void k_q_schema_emit(QView q, QSchema s, SchemaOut o, u32 names, Arr<u32> sort_keys) {
    const u32 j = blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    u64 off = 0, len = 0, w = 0;
    bool wide = false;
    if (j < s.n) {
        const u32 first = s.table[s.slot[j]];
        const u32 code = s.flag[first];
        sort_keys[j] = code * (u32)SJHIP_SCHEMA_TYPES + s.cls[j];
        if (first == j) {
            off = s.len[j];
            len = s.len[j + 1u] - off;
            o.name_off[code] = off;
            o.first_row[code] = s.parent[j];
            if (len) {
                w = q.tape[s.idx[j] - 2];
                wide = !(len <= COL_SHORT);  // (a short name by its lane, a long one by the wave, below)
                if (!wide) copy_bytes(arr_at(o.name_data, off, len), str_bytes(q, w, len), len, 0, 1);
            }
        }
        if (j == 0) o.name_off[names] = s.len[s.n];
    }
    wave_copy_strings(q, o.name_data, wide, off, len, w, lane);
}
// keys: the n sorted keys.  lo[k] = where the run of key k begins, hi[k] = where it ends (both stay 0 for a key that does not occur)
__global__ __launch_bounds__(256) void k_q_schema_bounds(Arr<const u32> keys, u32 n, Arr<u64> lo, Arr<u64> hi) {
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const u32 k = keys[i];
    if (i == 0 || keys[i - 1] != k) lo[k] = i;
    if (i + 1u == n || keys[i + 1] != k) hi[k] = (u64)i + 1u;
}
// counts: the run ends on entry, the run lengths on exit
__global__ __launch_bounds__(256) void k_q_schema_counts(Arr<const u64> lo, u32 m, Arr<u64> counts) {
    const u32 k = blockIdx.x * 256 + threadIdx.x;
    if (k < m) counts[k] = counts[k] - lo[k];
}


// ---- row predicates: keep the rows whose element at a path satisfies a test (sjhip_where_path) -----------------------------------
// A predicate narrows the row index: the rows of the selection -- or, without one, the root values of the records -- that satisfy
// it are compacted, in document order, into a new index, and every record keeps the matching ones among the rows it owned.
//   k_q_where_mark      one lane per current row: FindElement (an empty path: the row's value itself) and element_is, XORed with
//                       NOT; the flag of the row, and the kept rows of its 1024-row tile counted from the wave's ballot (one atomic
//                       per wave: no pass reads the flags back to sum them)
//   k_tw_scan_sums      the kept rows in front of every tile, and the total -- the one value the host waits for: the arena of a
//                       new selection is reserved for it
//   k_q_where_apply     per tile: the exclusive prefix of its flags; pre[i] = the kept rows in front of row i; row_value(q, i) of
//                       every kept row goes to its prefix in the NEW index (without a selection this materialises rec_open + 1)
//   k_q_where_offsets   one lane per record: its new row offset = pre[] at its old one (without a selection record r owned row r
//                       alone); the status copied, or OK
// The new index and the new offsets are built in the work arena and copied into d_rows behind the kernels (stream order): the old
// index is read by other blocks while the new one is produced, so it cannot be compacted in place.  No lane's work grows with
// the rows of a record.
struct QWhere {
    Arr<u8> flag;                 // [n] 1: row i is kept
    Arr<u32> pre;                 // [n] the kept rows in front of row i
    unsigned long long *tiles;    // [tiles] kept rows of the tile -> their exclusive prefix
    Arr<u64> index;               // [kept] the new row index (null while the rows are counted)
    Arr<const u64> old_off;       // [records + 1] the row offsets of the selection in force; null: record r owns row r
    const u8 *old_status;         // [records] its statuses (with old_off)
    Arr<u64> off;                 // [records + 1] the new row offsets
    u8 *status;                   // [records]
};
__global__ __launch_bounds__(256) void k_q_where_mark(QView q, QPath pth, int op, u64 want, u32 negate, QWhere w) {
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    bool keep = false;
    if (i < q_rows(q)) {
        keep = (pth.n ? record_is(q, pth, i, op, want) : element_is(q, row_value(q, i), op, want)) != (negate != 0);
        w.flag[i] = keep ? 1 : 0;
    }
    const u64 b = __ballot(keep);  // (the 64 rows of a wave lie in one tile)
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&w.tiles[i / QTILE], (unsigned long long)__popcll(b));
}
// ... by the row's NAME (sjhip_where_row_names): the rows are object members (sjhip_unnest_members), the name of row i is the string
// whose tag word lies two words in front of its value, and the test is element_is on that string
__global__ __launch_bounds__(256) void k_q_names_mark(QView q, int op, u64 want, u32 negate, QWhere w) {
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    bool keep = false;
    if (i < q_rows(q)) {
        keep = element_is(q, row_value(q, i) - 2u, op, want) != (negate != 0);
        w.flag[i] = keep ? 1 : 0;
    }
    const u64 b = __ballot(keep);  // (the 64 rows of a wave lie in one tile)
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&w.tiles[i / QTILE], (unsigned long long)__popcll(b));
}
// ... and the names as a string column (sjhip_extract_row_names): k_q_col_len's place in front of the column's scan and gather --
// the element is the name's string, every status is OK; entry n has length 0
__global__ __launch_bounds__(256) void k_q_names_len(QView q, QCol c) {
    const u32 r = blockIdx.x * 256 + threadIdx.x;
    if (r >= q_rows(q)) {
        if (r == q_rows(q)) c.off[r] = 0;
        return;
    }
    const u64 v = row_value(q, r) - 2u;
    c.idx[r] = v;
    c.off[r] = q.tape[v + 1];
    c.status[r] = (u8)SJHIP_COL_OK;
}
// ... by SEVERAL tests (sjhip_where_paths): the mark of a plan of predicates (sj_where.h).  One lane per row runs table_walk over
// the predicates' paths -- every member of the row is met once, however many tests look at it --, the sink evaluates the predicate
// of the column on the element it is handed (element_is on the predicate's own value span; SJHIP_PATH_NOT_*: false) into one bit
// of a truth mask, the predicates with an empty path test the row's value, and the program folds the mask into the flag.  The flag
// and the tile count leave as in k_q_where_mark; with `count` set (sjhip_count_where_paths) the ballot is added to that one
// counter instead and nothing else is written.  The resume stack is the table kernel's: LDS, one column per lane.
struct WhereSink {
    const QView &q;
    const WherePlan &p;
    u32 truth;
    __device__ __forceinline__ void test(u32 k, u64 v) {  // predicate k on the element at v
        if (element_is(q, v, p.op[k], p.want[k], q.val + p.val_b[k], p.val_n[k])) truth |= 1u << k;
    }
    __device__ __forceinline__ void operator()(u32 c, u64 v) {
        if (v < SJHIP_PATH_NOT_OBJECT) test(p.pred_of_col[c], v);
    }
};
static_assert(sizeof(QView) + sizeof(WherePlan) + sizeof(QWhere) + 8 <= 4096,
              "k_q_where_multi_mark: the view and the plan travel as kernel arguments (4 KiB)");
__global__ __launch_bounds__(256) void k_q_where_multi_mark(QView q, WherePlan p, QWhere w, unsigned long long *count) {
    __shared__ u32 s_stack[TABLE_STACK_WORDS * 256];
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    bool keep = false;
    if (i < q_rows(q)) {
        const u64 v0 = row_value(q, i);
        const TableView view = {q};
        WhereSink sink = {q, p, 0u};
        if (p.pl.n_cols) table_walk(view, p.pl, v0, s_stack + threadIdx.x, 256u, sink);
        if (p.empty)
            for (u32 k = 0; k < p.n_preds; k++)
                if ((p.empty >> k) & 1u) sink.test(k, v0);
        keep = where_program_eval(p.program, p.program_len, sink.truth);
        if (!count) w.flag[i] = keep ? 1 : 0;
    }
    if (count) {
        count_ballot(keep, count);
        return;
    }
    const u64 b = __ballot(keep);  // (the 64 rows of a wave lie in one tile)
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&w.tiles[i / QTILE], (unsigned long long)__popcll(b));
}
// ... by MEMBERSHIP in a set of values (sjhip_where_path_in: a semi-join, and with NOT an anti-join).  The set is the caller's:
// uploaded as it came, hashed and entered into an open-addressing table of value indices (sj_wherein.h) by
//   k_q_in_build   one lane per value: the grouping's hash of the value (group_hash_bytes / group_hash_int: a row's key hashes as
//                  in the grouping) is stored for the probes, and the value claims a slot of the u32 table of
//                  group_table_capacity(n_values) slots -- k_q_group_insert's loop: compare-and-swap on an empty slot, an equal
//                  value already there ends the probe and the smaller index stays (atomicMin), anything else probes on.  Occupants
//                  are compared by VALUE here, not by hash[]: the values lay on the device before the kernel began, the hash of
//                  another lane's value may not.  Every access to the table is a device-scope atomic; no locks, no spinning,
//                  bounded by the capacity.
//   k_q_in_mark    k_q_where_mark's place in where_build, one lane per row: FindElement (an empty path: the row's value), the
//                  conversion of the EQ_* operator of the set's kind -- the string's unescaped bytes wherever they lie, element_to
//                  for INT / UINT; no usable key: no match --, the hash, and the probe from the home slot to the first empty one:
//                  at an occupied slot the stored hash first, then the value (a string's length before any byte).  The cost of a
//                  row is its walk, its hash and a chain whose expected length does not depend on the size of the set (load <= 1/2).
//                  The flag and the tile count leave as in k_q_where_mark, with `count` set the ballot goes to that one counter
//                  and nothing else is written (k_q_where_multi_mark's rule).  An empty set has no table: every flag is `negate`.
// The string probe is inlined: the kernel then needs k_q_where_mark's registers and no scratch on both builds, whereas a call
// would have to hand the view and the set over in memory -- kernel arguments copied to scratch (64 bytes per lane in the product
// build, the whole view in the bounds-checked one).  tests/test_where_in_kernel_resources.py holds both kernels to that.
struct InAtomicTable {
    __device__ __forceinline__ u32 load(u32 *cell) const { return __hip_atomic_load(cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ u32 claim(u32 *cell, u32 j) const { return atomicCAS(cell, GROUP_NONE, j); }
    __device__ __forceinline__ void lower(u32 *cell, u32 j) const { (void)atomicMin(cell, j); }
};
static_assert(IN_KIND_STRING == SJHIP_COL_STRING && IN_MAX_STRING == (u32)QMAX, "sj_wherein.h takes the header's kind and EQ_STRING's limit");
__global__ __launch_bounds__(256) void k_q_in_build(InSet s) {
    const u32 j = blockIdx.x * 256 + threadIdx.x;
    if (j >= s.n) return;
    const u64 h = in_value_hash(s, j);
    s.hash[j] = h;
    (void)in_insert(s, j, h, InAtomicTable());
}
__device__ __forceinline__ bool in_string_matches(const QView &q, const InSet &s, u64 w, u64 len) {
    const u8 *const p = str_bytes(q, w, len);
    return in_probe(s, group_hash_bytes(p, len), 0, p, len);
}
__device__ __forceinline__ bool in_element_matches(const QView &q, const InSet &s, u64 v) {
    if (s.kind == SJHIP_COL_STRING) {
        const u64 w = q.tape[v];
        if ((u32)(w >> 56) != '"') return false;
        const u64 len = q.tape[v + 1];
        return len <= IN_MAX_STRING && in_string_matches(q, s, w, len);  // (no value of a set is longer)
    }
    u64 x;
    return element_to(q, v, s.kind, &x) == SJHIP_COL_OK && in_probe(s, group_hash_int(x), x, nullptr, 0);
}
static_assert(sizeof(QView) + sizeof(QPath) + sizeof(InSet) + sizeof(QWhere) + 16 <= 4096, "k_q_in_mark: its arguments travel as kernel arguments (4 KiB)");
__global__ __launch_bounds__(256) void k_q_in_mark(QView q, QPath pth, InSet s, u32 negate, QWhere w, unsigned long long *count) {
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    bool keep = false;
    if (i < q_rows(q)) {
        bool in = false;
        if (s.n) {
            const u64 v = pth.n ? record_find_path(q, pth, i) : row_value(q, i);
            in = v < SJHIP_PATH_NOT_OBJECT && in_element_matches(q, s, v);
        }
        keep = in != (negate != 0);
        if (!count) w.flag[i] = keep ? 1 : 0;
    }
    if (count) {
        count_ballot(keep, count);
        return;
    }
    const u64 b = __ballot(keep);  // (the 64 rows of a wave lie in one tile)
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&w.tiles[i / QTILE], (unsigned long long)__popcll(b));
}
__global__ __launch_bounds__(QT) void k_q_where_apply(QView q, QWhere w) {
    __shared__ unsigned long long s_w[QT / 64];
    const u32 n = q_rows(q), base = blockIdx.x * QTILE + threadIdx.x * QI;
    u32 f[QI], sum = 0;
#pragma unroll
    for (int k = 0; k < QI; k++) {
        f[k] = base + k < n ? w.flag[base + k] : 0u;
        sum += f[k];
    }
    u64 at = w.tiles[blockIdx.x] + block_excl_sum(sum, s_w, (int)threadIdx.x, nullptr);
#pragma unroll
    for (int k = 0; k < QI; k++) {
        if (base + k >= n) break;
        w.pre[base + k] = (u32)at;
        if (f[k]) w.index[at++] = row_value(q, base + k);
    }
}
__global__ __launch_bounds__(256) void k_q_where_offsets(QView q, QWhere w, u64 kept) {
    const u32 r = blockIdx.x * 256 + threadIdx.x;
    if (r > q.R) return;
    const u64 old = w.old_off ? w.old_off[r] : (u64)r;
    w.off[r] = old < q_rows(q) ? (u64)w.pre[old] : kept;  // (the records behind the last row: everything kept lies in front)
    w.status[r] = w.old_off ? w.old_status[r] : (u8)SJHIP_COL_OK;
    if (r == q.R) w.off[r + 1] = kept;
}

// ---- filter rows: the selected rows as a self-contained (Tape, Strings.B) (sjhip_filter_rows) ---------------------------------------
// The materialiser of the row selection: every selected row that is a container becomes a record of a new result -- an opening
// root, the row's words [v, payload(tape[v])) with every stored index rebased, a closing root -- and the string bytes of the rows
// are laid end to end: what ParseND returns for the document whose lines are the texts of those rows.  A scalar row has no such
// record (stage 1 rejects a scalar line): it is left out and counted.
//   k_q_frows_measure     per row: its output words (0: a scalar), the Strings.B offset of its first string and the end of its
//                         last one.  Rows do not tile the tape -- what lies between two rows belongs to neither -- so the last
//                         string is found by classifying the row's own words: a row of up to FROWS_SHORT words by its lane, entry
//                         by entry; every longer row of the wave's 64 by the whole wave in turn (wave_each), 64 words per step,
//                         tags told from raw words by the span walk of sj_tapewalk.h (tw_walk_span; the row's value is the first
//                         word of an entry), the first and the last string of a step from one ballot.  Emitted and skipped rows
//                         are counted from the wave's ballots.
//   scan                  exclusive prefixes of the words and of the string bytes over the rows (the filter's tile pattern:
//                         sums -> k_tw_scan_sums -> apply); both totals and both counts reach the host in one copy
//   k_q_frows_copy        one wave per emitted row: wave_copy_record, the rebasing copy it shares with k_q_copy
// A row owns Strings.B from its first string to the end of its last: strings lie in document order and a row is one stretch of the
// document, so everything in between is a string of the row (keys and nested strings included).
static constexpr u32 FROWS_SHORT = 128;  // words of a row its lane walks alone
struct QFRows {
    Arr<u32> words;      // [n] output words of the row (0: a scalar) -> their exclusive prefix = new index of its opening root
    Arr<u32> first_str;  // [n] Strings.B offset of its first string (NONE32: it has none)
    Arr<u32> s_len;      // [n] bytes of Strings.B it owns (0 for a scalar)
    Arr<u32> s_pre;      // [n] their exclusive prefix = new Strings.B offset of its first string
    unsigned long long *tw, *tb;  // [tiles] tile sums of words / s_len -> their exclusive prefixes
    unsigned long long *totals;   // [0] words, [1] bytes (the scans); [4] rows emitted, [5] scalar rows skipped (the measure)
};
__device__ __forceinline__ u32 str_offset(u64 w) { return (u32)(w & (STRINGBUFBIT - 1)); }  // (every string is copied: the host checked)
// the strings of the row [v, end) by one lane: entry by entry (a number's second word is stepped over)
__device__ __forceinline__ void lane_row_strings(const QView &q, u64 v, u64 end, u32 *first, u32 *last_end) {
    u64 last = 0;
    u32 fs = NONE32;
    for (u64 i = v; i < end;) {
        const u64 w = q.tape[i];
        if ((w >> 56) == '"') {
            if (fs == NONE32) fs = str_offset(w);
            last = i;
        }
        i += two_word_tag(w) ? 2 : 1;
    }
    *first = fs;
    *last_end = fs == NONE32 ? 0u : str_offset(q.tape[last]) + (u32)q.tape[last + 1];
}
// ... and by the whole wave, 64 words per step (arguments and results wave-uniform)
__device__ __forceinline__ void wave_row_strings(const QView &q, u64 v, u64 end, int lane, u32 *first, u32 *last_end) {
    u32 fs = NONE32, le = 0;
    tw_walk_span(q.tape, v, end - v, lane, [&](u64 i, u64 w, bool in, bool raw) {
        const bool str = in && !raw && (w >> 56) == '"';
        // (a string's length word may lie in the next step: its own lane reads it; it lies inside the row, a close follows it)
        const u32 mine = str ? str_offset(w) + (u32)q.tape[v + i + 1] : 0u;
        const u64 sm = __ballot(str);
        if (sm) {
            if (fs == NONE32) fs = wave_bcast(str_offset(w), __ffsll((unsigned long long)sm) - 1);
            le = wave_bcast(mine, 63 - __builtin_clzll(sm));
        }
    });
    *first = fs;
    *last_end = le;
}
__global__ __launch_bounds__(256) void k_q_frows_measure(QView q, QFRows o) {
    const u32 r = blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool have = r < q_rows(q);
    u64 v = 0, end = 0;
    u32 first = NONE32, last_end = 0;
    bool box = false, wide = false;
    if (have) {
        v = row_value(q, r);
        const u64 w = q.tape[v];
        const u32 t = (u32)(w >> 56);
        box = t == '{' || t == '[';
        if (box) {
            end = w & TW_PAYLOAD;  // behind the matching close
            wide = end - v > FROWS_SHORT;
            if (!wide) lane_row_strings(q, v, end, &first, &last_end);
        }
    }
    wave_each(wide, [&](int j) {  // the wave's long rows, one after another
        u32 f_j, l_j;
        wave_row_strings(q, wave_bcast(v, j), wave_bcast(end, j), lane, &f_j, &l_j);
        if (lane == j) {
            first = f_j;
            last_end = l_j;
        }
    });
    if (have) {
        o.words[r] = box ? (u32)(end - v) + 2u : 0u;
        o.first_str[r] = first;
        o.s_len[r] = first == NONE32 ? 0u : last_end - first;
    }
    count_ballot(box, &o.totals[4]);
    count_ballot(have && !box, &o.totals[5]);
}
__global__ __launch_bounds__(QT) void k_q_frows_tile_sums(QFRows o, u32 n) {
    tile_sums(arr_raw(o.words), n, o.tw);
    tile_sums(arr_raw(o.s_len), n, o.tb);
}
__global__ __launch_bounds__(QT) void k_q_frows_tile_apply(QFRows o, u32 n) {
    tile_apply(arr_raw(o.words), arr_raw(o.words), n, o.tw);
    tile_apply(arr_raw(o.s_len), arr_raw(o.s_pre), n, o.tb);
}
__global__ __launch_bounds__(256) void k_q_frows_copy(QView q, QFRows o, Arr<u64> out_tape, Arr<u8> out_strings) {
    const u32 r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= q_rows(q)) return;  // wave-uniform, like the next one
    const u64 v = row_value(q, r), w0 = q.tape[v];
    const u32 t0 = (u32)(w0 >> 56);
    if (t0 != '{' && t0 != '[') return;
    // the row's own words, up to its matching close
    wave_copy_record(q, v, (w0 & TW_PAYLOAD) - v, o.words[r], o.first_str[r], o.s_len[r], o.s_pre[r], threadIdx.x & 63, out_tape, out_strings);
}

// ---- groups: the distinct keys at a path, a code per row, aggregates per key (sjhip_group_path, sjhip_group_paths) -------------------
// "group by": the key of a row is a tuple with one entry per key column -- FindElement(the column's path) + Iter.StringBytes, Iter.Int,
// Iter.Uint or Iter.Bool; two rows in a group are in one group iff their tuples are equal entry by entry, and groups are numbered by
// first occurrence -- so codes, dictionary, first rows and group sizes are decided by the input alone, not by the hash or by which lane
// came first.  sjhip_group_path is the tuple of one column.  All on the device, kernel boundaries do the ordering:
//   k_q_group_keys     once per column, one lane per row: the walk, the conversion, status[c][r] and kidx[c][r] (STRING: the tape
//                      index; the other kinds: the value) and the key's 64-bit hash (sj_group.h: 8 bytes per step).  A long key is
//                      hashed -- and later compared -- by its lane alone: the keys this serves (a make, a language, a screen name)
//                      are short.
//   k_q_group_insert   the dictionary: an open-addressing table of row numbers (empty: GROUP_NONE), capacity a power of two >= twice
//                      the rows, linear probing.  A row claims an empty slot by compare-and-swap; on an occupied one it compares its
//                      key with the occupant ROW's key -- the hash first, then the entries (group_tuples_equal).  What it reads of
//                      the occupant -- status, kidx, hash, tape, Strings.B, message -- was written before this kernel began and is
//                      read-only here, so the slot word is all that is communicated.  On equality it lowers the slot to the smaller
//                      row (atomicMin, skipped when the occupant is smaller already: a handful of distinct keys would otherwise draw
//                      every row's atomic to a handful of addresses), else probes on.  The occupant only ever changes to a smaller
//                      row with an EQUAL key, so a comparison stays valid whatever happens to the slot afterwards, and a key always
//                      ends in the first slot of its probe sequence that did not hold a different key.  Every access to the table
//                      here is a device-scope atomic (a plain load may be served from another XCD's L2).  No lane waits for
//                      another: nothing locks, nothing spins, and because the capacity exceeds the rows every probe sequence ends
//                      (the loop is bounded by the capacity besides).
//   k_q_group_first    behind the boundary: row r is the first of its group iff table[slot[r]] == r -> flag; per STRING column the
//                      length of a first row's key (0 without one).  Exclusive scans (the tile pattern of sj_tapewalk.h:
//                      k_q_group_tile_sums, k_tw_scan_sums, k_q_group_tile_apply, once per scanned array) number the groups and
//                      place every STRING column's keys; the totals are the groups, the rows in a group -- counted beside the
//                      flags' tile sums: one atomic per wave on one address took as long as the table -- and the columns' key bytes.
//   k_q_group_emit     once per column: the column's status of every row, and by the first rows their group's entry -- key_ok, and
//                      the value, or the offset and the bytes (a short key by the lane, a long one by the wave, like the string
//                      column).  The launch of column 0 writes codes, first_row and the sort's keys as well.
//   the sort           the stable radix sort of sj_sort.h: the rows by code, position i being row i, over only as many low digits as
//                      the group count has (group_pass_mask).  Rows in no group carry the code `groups` and end behind all.
//   k_q_group_bounds   in the sorted sequence a position whose code differs from the one in front begins a group: the group offsets;
//   k_q_group_counts   their differences are group_rows -- no contended atomics anywhere.
// The aggregates are the segmented reduction above with the sorted rows as QAgg::perm and the group offsets as the row offsets
// (AGG_OFFS), once per value column: groups in the place of records, so association, 128-bit sums and min / max keys are the tested ones.
// Several keys add three things.  The tuple's hash is folded column by column (group_tuple_fold: order-dependent; the first column's
// hash begins it, so one column hashes as itself).  A column that carries SJHIP_GROUP_NULL_KEY turns a status that is not OK into
// the entry "no key" (GROUP_NO_KEY_HASH; equal to "no key" only); without the flag such a row is in no group -- the `in` byte.  And
// every column is one more walk of every row and one more emit: DESIGN.md (Several keys).
struct QGroup {
    u32 n, mask, n_cols;
    u32 kinds;       // 4 bits per column: its SJHIP_COL_* kind
    u32 null_mask;   // bit c: column c carries SJHIP_GROUP_NULL_KEY
    u32 str_slot;    // 4 bits per column: which of the length arrays a STRING column has
    u32 tiles;
    Arr<u8> status;  // [n_cols * n] column-major: the status of row r on column c at c * n + r
    Arr<u64> kidx;   // [n_cols * n] STRING: tape index of the key element; the other kinds: the value
    Arr<u64> hash;   // [n] the tuple hash, complete behind the last column's launch
    Arr<u8> in;      // [n] 1: the row is in a group
    Arr<u32> slot;   // [n] the slot the row ended in
    Arr<u32> table;  // [mask + 1] row numbers
    Arr<u32> flag;   // [n + 1] 1 at the first row of a group -> exclusive prefix: the group's number
    Arr<u64> len;    // [STRING columns * (n + 1)] bytes of a first row's key -> their offset among the column's entries
    unsigned long long *tiles_f, *tiles_o, *tiles_l;  // [tiles] flags / rows in a group; [STRING columns * tiles] lengths
};
struct GroupOut {  // column c of the product (d_group), and what the launch of column 0 writes beside it: see group_layout
    Arr<u64> key_off;    // [groups + 1] STRING
    Arr<u8> key_bytes;   // [key bytes] STRING
    Arr<u64> key_val;    // [groups] INT, UINT
    Arr<u8> key_u8;      // [groups] BOOL
    Arr<u8> key_ok;      // [groups]
    Arr<u8> status;      // [n]
    Arr<u64> first_row;  // [groups]
    Arr<u32> codes;      // [n]
};
__device__ __forceinline__ int group_kind(const QGroup &g, u32 c) { return (int)((g.kinds >> (4u * c)) & 15u); }
__device__ __forceinline__ u64 group_len_at(const QGroup &g, u32 c) { return (u64)((g.str_slot >> (4u * c)) & 15u) * ((u64)g.n + 1u); }
__device__ __forceinline__ bool group_tuples_equal(const QView &q, const QGroup &g, u32 a, u32 b) {
    for (u32 c = 0; c < g.n_cols; c++) {
        const u64 at = (u64)c * g.n;
        const bool ok = g.status[at + a] == SJHIP_COL_OK;
        if (ok != (g.status[at + b] == SJHIP_COL_OK)) return false;
        if (!ok) continue;  // "no key" equals "no key"
        const u64 ka = g.kidx[at + a], kb = g.kidx[at + b];
        if (group_kind(g, c) != SJHIP_COL_STRING) {
            if (ka != kb) return false;
            continue;
        }
        const u64 len = q.tape[ka + 1];
        if (len != q.tape[kb + 1]) return false;
        if (!group_bytes_equal(str_bytes(q, q.tape[ka], len), str_bytes(q, q.tape[kb], len), len)) return false;
    }
    return true;
}
__global__ __launch_bounds__(256) void k_q_group_keys(QView q, QPath pth, QGroup g, u32 c) {
    const u32 r = blockIdx.x * 256 + threadIdx.x;
    if (r >= g.n) return;
    const int kind = group_kind(g, c);
    const u64 v = pth.n ? record_find_path(q, pth, r) : row_value(q, r);  // (no keys: the row's own value)
    int st;
    u64 k = 0, h = GROUP_NO_KEY_HASH;
    if (v >= SJHIP_PATH_NOT_OBJECT) st = path_status(v);
    else if (kind == SJHIP_COL_STRING) {
        u64 len = 0;
        st = element_text_len(q, v, false, &len);
        if (st == SJHIP_COL_OK) {
            k = v;
            h = group_hash_bytes(str_bytes(q, q.tape[v], len), len);
        }
    } else {
        st = element_to(q, v, kind, &k);
        if (st == SJHIP_COL_OK) h = group_hash_int(k);
        else k = 0;
    }
    const u64 at = (u64)c * g.n + r;
    g.status[at] = (u8)st;
    g.kidx[at] = k;
    g.hash[r] = c ? group_tuple_fold(g.hash[r], h) : h;
    const bool keeps = st == SJHIP_COL_OK || ((g.null_mask >> c) & 1u);
    if (c == 0) g.in[r] = keeps ? 1 : 0;
    else if (!keeps) g.in[r] = 0;
}
__global__ __launch_bounds__(256) void k_q_group_insert(QView q, QGroup g) {
    const u32 r = blockIdx.x * 256 + threadIdx.x;
    if (r >= g.n || !g.in[r]) return;
    const u64 h = g.hash[r];
    u32 s = (u32)h & g.mask;
    for (u32 step = 0; step <= g.mask; step++, s = (s + 1u) & g.mask) {
        u32 *const cell = &g.table[s];
        u32 cur = __hip_atomic_load(cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == GROUP_NONE) {
            cur = atomicCAS(cell, GROUP_NONE, r);
            if (cur == GROUP_NONE) break;  // claimed
        }
        if (cur == r) break;
        if (g.hash[cur] == h && group_tuples_equal(q, g, r, cur)) {
            if (cur > r) (void)atomicMin(cell, r);
            break;
        }
    }
    g.slot[r] = s;
}
// (one lane per entry of the n + 1: entry n is 0, the scans leave the totals there)
__global__ __launch_bounds__(256) void k_q_group_first(QView q, QGroup g) {
    const u32 r = blockIdx.x * 256 + threadIdx.x;
    if (r > g.n) return;
    const bool first = r < g.n && g.in[r] && g.table[g.slot[r]] == r;
    g.flag[r] = first ? 1u : 0u;
    for (u32 c = 0; c < g.n_cols; c++) {
        if (group_kind(g, c) != SJHIP_COL_STRING) continue;
        const u64 at = (u64)c * g.n + r;
        g.len[group_len_at(g, c) + r] = first && g.status[at] == SJHIP_COL_OK ? q.tape[g.kidx[at] + 1] : 0ull;
    }
}
// round 0: the flags, the rows in a group counted beside them, and the length array 0 (the first STRING column's, if there is one);
// round s >= 1: the length array s
__global__ __launch_bounds__(QT) void k_q_group_tile_sums(QGroup g, u32 m, u32 round) {
    __shared__ unsigned long long s_w[QT / 64];
    if (round) {
        tile_sums(arr_at(g.len, (u64)round * m, m), m, g.tiles_l + (size_t)round * g.tiles);
        return;
    }
    tile_sums(arr_at(g.flag, 0, m), m, g.tiles_f);
    if (g.len) tile_sums(arr_at(g.len, 0, m), m, g.tiles_l);
    const u32 base = blockIdx.x * QTILE + threadIdx.x * QI;
    unsigned long long in = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < QI; k++)
        if (base + k < g.n && g.in[base + k]) in++;
    (void)block_excl_sum(in, s_w, (int)threadIdx.x, &tot);
    if (threadIdx.x == 0) g.tiles_o[blockIdx.x] = tot;
}
__global__ __launch_bounds__(QT) void k_q_group_tile_apply(QGroup g, u32 m, u32 round) {
    if (round || g.len) {
        u64 *const len = arr_at(g.len, (u64)round * m, m);
        tile_apply(len, len, m, g.tiles_l + (size_t)round * g.tiles);
    }
    if (round) return;
    u32 *const flag = arr_at(g.flag, 0, m);
    tile_apply(flag, flag, m, g.tiles_f);
}
// (sort_keys: the first pass's input -- the row's code, or `groups` for a row in no group; written by the launch of column 0)
__global__ __launch_bounds__(256) void k_q_group_emit(QView q, QGroup g, GroupOut o, u32 groups, Arr<u32> sort_keys, u32 c) {
    const u32 r = blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int kind = group_kind(g, c);
    u64 off = 0, len = 0, w = 0;
    bool wide = false;
    if (r < g.n) {
        const u64 at = (u64)c * g.n + r;
        const u8 st = g.status[at];
        u32 code = GROUP_NONE, first = GROUP_NONE;
        if (g.in[r]) {
            first = g.table[g.slot[r]];
            code = g.flag[first];
        }
        if (c == 0) {
            o.codes[r] = code;
            sort_keys[r] = code == GROUP_NONE ? groups : code;
            if (first == r) o.first_row[code] = r;
        }
        o.status[r] = st;
        if (first == r) {
            const bool ok = st == SJHIP_COL_OK;
            o.key_ok[code] = ok ? 1 : 0;
            if (kind == SJHIP_COL_STRING) {
                const u64 la = group_len_at(g, c) + r;
                off = g.len[la];
                len = g.len[la + 1] - off;  // (0 without a key)
                o.key_off[code] = off;
                if (len) {
                    w = q.tape[g.kidx[at]];
                    wide = len > COL_SHORT;
                    if (!wide) copy_bytes(arr_at(o.key_bytes, off, len), str_bytes(q, w, len), len, 0, 1);
                }
            } else if (kind == SJHIP_COL_BOOL) o.key_u8[code] = (u8)g.kidx[at];
            else o.key_val[code] = g.kidx[at];
        }
        if (r == 0 && kind == SJHIP_COL_STRING) o.key_off[groups] = g.len[group_len_at(g, c) + g.n];
    }
    wave_copy_strings(q, o.key_bytes, wide, off, len, w, lane);
}
// keys: the sorted codes; the first n_ok positions are the rows with a key.  off[g] = the position group g begins at, off[groups] = n_ok
__global__ __launch_bounds__(256) void k_q_group_bounds(Arr<const u32> keys, u32 n_ok, u32 groups, Arr<u64> off) {
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_ok) return;
    const u32 k = keys[i];
    if (i == 0 || keys[i - 1] != k) off[k] = i;
    if (i == 0) off[groups] = n_ok;
}
__global__ __launch_bounds__(256) void k_q_group_counts(Arr<const u64> off, u32 groups, Arr<u64> group_rows) {
    const u32 g = blockIdx.x * 256 + threadIdx.x;
    if (g < groups) group_rows[g] = off[g + 1] - off[g];
}

// ---- order: the rows ranked by key columns at paths, the first `limit` of them kept (sjhip_order_path, _strings, sjhip_order_paths) ---
// The order is the one a stable sort by the tuple of up to SJHIP_ORDER_MAX_KEYS columns gives: per column the rows with an OK key
// ascending by it (a number by agg_key, a string by bytes.Compare on the unescaped key bytes; descending: by the complement), equal
// keys in row order, the rows without one behind them, tied.  A single-key call is the one-column case.  The selection is narrowed
// to the rows of rank < limit as a row predicate would narrow it (the second half of where_build: k_q_where_apply,
// k_q_where_offsets), so it stays in document order; the order itself is a product of its own (d_order).
// `perm` holds the rows in rank order as far as it is known.  A CLASS is a run of positions of perm whose rows tie on everything
// looked at so far; the ACTIVE entries are the members of the classes that are not finished, held as (row, position, class) in
// ascending position, so classes are numbered in position order and each owns a contiguous stretch of positions.  A string key has
// any length, so a string column is refined most-significant chunk first, STRORD_CHUNK = 7 key bytes per round (strord_chunk,
// sj_order.h); a numeric column is one round.  The rows without an OK key on a column lie behind the others of their class and tie
// there, so they still meet the later columns: the sort by class takes mkord_class_key = class << 1 | missing.  Entries leave a
// column at different rounds, so what the next column works on is not queued but rebuilt from a boundary byte per position,
// bnd[p] = 1 where a class begins (bnd[n] = 1).
//   k_q_order_init     all n rows active in row order, one class; perm = the rows; bnd = 1 at 0 and at n
//   (a single-key call starts elsewhere: no later column waits for its rows without a key, so behind k_q_order_keys they are
//   parked -- the scan of the tiles' OK rows, then k_q_order_park: the OK rows to the front, active in one class, the others behind
//   them for good -- and the rounds sort by chunk key alone.  A numeric key has no rounds: k_q_order_park writes the (key, row)
//   pairs, k_q_order_fold the AND / OR of the keys, and one sort of the OK rows is the order.  Measured, DESIGN.md: the missing bit
//   costs a single-key call a second sort, and a numeric one the chunk and place kernels, that it has no use for)
//   column c:
//   k_q_order_keys     one lane per ACTIVE entry: path, status and, for a numeric column, the sort key agg_key (complemented for
//                      a descending column); for a string column the tape index of the element, and the tile's longest key.  A column
//                      behind the first walks only the rows that still tie
//   round j (a numeric column has one, a string column strord_max_rounds(longest) at most):
//   k_q_order_chunks   the round's chunk key of every active entry -- the numeric key, or the string's chunk at byte 7 j; 0 for a
//                      missing row -- and its class key; per tile the AND and the OR of the chunk keys of the OK rows and of the class
//                      keys (block_and_or: wave reductions joined through LDS, one plain store per tile and value).  Launched for the
//                      active count of the round before, an upper bound; the count itself is read on the device
//   k_q_order_fold     one block: the ANDs and ORs over the tiles (round 0 of a column: its longest key as well) -> the host's one
//                      copy per round: the active count, and the pass plans of the two sorts (order_pass_mask: a digit whose bits
//                      are equal in all keys takes no pass; a round without missing rows plans no extra digit)
//   the sort           stable by (class key, chunk key), least significant first: sort_enqueue<u64> over the chunk-key digits that
//                      vary, then k_q_order_classes gathers the class keys behind the sorted entries and sort_enqueue<u32> takes
//                      their varying digits (one class without missing rows: skipped)
//   k_q_order_place    the i-th sorted entry goes to the i-th active position (all members of a class are active or none is, so
//                      every class lands on its own stretch); a HEAD differs in (class key, chunk key) from the entry in front and
//                      sets bnd at its position; an entry STAYS in the column iff mkord_stays: it has a key, its new class has company
//                      and its chunk was full (count 7: a class whose chunk ended is a run of equal keys, finished in row order
//                      because the sort is stable).  The tile sums of both flags
//   scan, k_q_order_compact  (string columns) new class numbers (the heads up to and including the entry) and the entries that
//                      stay, with their positions, into the other buffer -- until nothing is active
//   between columns:
//   k_q_order_bounds   the tile sums of bnd and of "not alone in its class", !(bnd[p] && bnd[p + 1])
//   k_q_order_rebuild  behind their scan: the entries that are not alone, (perm[p], p, the heads up to and including p)
// Nothing active: the remaining columns are skipped.  Then
//   k_q_order_flag     the row at rank p is kept iff p < limit -> the flag of a row predicate; k_q_order_flag_sums its tile sums
//   k_q_order_emit     behind the narrowing: order[p] = pre[row(p)], the row's number in the new selection; its status on column 0
//                      (the only column every row is evaluated on) and, for sjhip_order_path, its value
// No atomics anywhere.
static_assert(ORDER_MAX_KEYS == SJHIP_ORDER_MAX_KEYS, "sj_order.h mirrors include/sjhip.h");
struct QOrder {
    u32 n;
    Arr<u8> status;                                 // [n] the key's status ON THE COLUMN AT WORK
    Arr<u64> kidx;                                  // [n] there: the sort key of a number, the tape index of a string element (OK rows)
    Arr<u32> perm;                                  // [n] the rows in rank order
    Arr<u32> row, pos, cls;                         // [n] each: the active entries of the round
    Arr<u32> row_out, pos_out, cls_out;             // [n] each: those of the next round (the host swaps the two sets)
    Arr<u64> chunk;                                 // [n] the round's chunk key of active entry i
    Arr<u32> ckey;                                  // [n] its class key
    Arr<u8> flags;                                  // [n] bit 0: head, bit 1: stays active -- of the i-th SORTED entry
    Arr<u8> bnd;                                    // [n + 1] 1 where a class begins
    unsigned long long *tiles_ok, *tiles_len;       // [tiles] the OK keys of the tile's entries (-> their prefix); its longest OK key
    unsigned long long *tiles_kand, *tiles_kor, *tiles_cand, *tiles_cor;  // [tiles] AND / OR of the chunk keys / of the class keys
    unsigned long long *tiles_head, *tiles_act;     // [tiles] heads / active entries of the tile -> their exclusive prefixes
    unsigned long long *totals;                     // ORDER_T_*
};
// totals: [4] the classes and [5] the active entries (k_q_order_init; k_tw_scan_sums of tiles_head / tiles_act), [6] the column's
// longest OK key, [8 .. 12) the AND / OR of the round's chunk keys, of its class keys
static constexpr int ORDER_T_HEADS = 4, ORDER_T_ACTIVE = 5, ORDER_T_LONGEST = 6, ORDER_T_ANDOR = 8, ORDER_T_WORDS = 12;
// all := the AND of every thread's `all`, any := the OR of every thread's `any`, in thread 0 of a block of QT threads: wave
// reductions, the waves joined through s_w
__device__ __forceinline__ void block_and_or(u64 &all, u64 &any, unsigned long long (*s_w)[QT / 64]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        all &= (u64)__shfl_xor((long long)all, s, 64);
        any |= (u64)__shfl_xor((long long)any, s, 64);
    }
    if (lane == 0) s_w[0][wave] = all, s_w[1][wave] = any;
    __syncthreads();
    if (tid == 0)
        for (int w = 1; w < QT / 64; w++) all &= s_w[0][w], any |= s_w[1][w];
}
// the maximum of every thread's x in thread 0 of a block of QT threads
__device__ __forceinline__ u64 block_max(u64 x, unsigned long long *s_w) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const u64 o = (u64)__shfl_xor((long long)x, s, 64);
        x = o > x ? o : x;
    }
    if (lane == 0) s_w[wave] = x;
    __syncthreads();
    if (tid == 0)
        for (int w = 1; w < QT / 64; w++) x = s_w[w] > x ? s_w[w] : x;
    return x;
}
__global__ __launch_bounds__(256) void k_q_order_init(QOrder o) {
    const u32 i = blockIdx.x * 256 + threadIdx.x, n = o.n;
    if (i >= n) return;
    o.perm[i] = i;
    o.row[i] = i;
    o.pos[i] = i;
    o.cls[i] = 1;
    o.bnd[i] = i == 0 ? 1 : 0;
    if (i == 0) {
        o.bnd[n] = 1;
        o.totals[ORDER_T_ACTIVE] = n;
    }
}
// active: where the device keeps the number of active entries (first: column 0, the entries are the n rows); kind:
// SJHIP_COL_FLOAT / INT / UINT or SJHIP_COL_STRING
__global__ __launch_bounds__(QT) void k_q_order_keys(QView q, QPath pth, QOrder o, int kind, u32 desc, u32 first,
                                                     const unsigned long long *active) {
    __shared__ unsigned long long s_len[QT / 64], s_ok[QT / 64];
    const int tid = threadIdx.x;
    const u32 m = first ? o.n : (u32)*active;
    u64 longest = 0;
    unsigned long long ok = 0, tot_ok = 0;
#pragma unroll 1
    for (int k = 0; k < QI; k++) {
        const u32 i = blockIdx.x * QTILE + k * QT + tid;
        if (i >= m) break;
        const u32 r = first ? i : o.row[i];
        const u64 v = pth.n ? record_find_path(q, pth, r) : row_value(q, r);  // (no keys: the row's own value)
        u64 x = 0, key = 0;
        int st;
        if (v >= SJHIP_PATH_NOT_OBJECT) st = path_status(v);
        else if (kind == SJHIP_COL_STRING) {
            st = element_text_len(q, v, false, &x);
            if (st == SJHIP_COL_OK) {
                key = v;
                longest = x > longest ? x : longest;
            }
        } else {
            st = element_to(q, v, kind, &x);
            if (st == SJHIP_COL_OK) {
                key = agg_key(x, kind);
                if (desc) key = ~key;
            }
        }
        o.status[r] = (u8)st;
        o.kidx[r] = key;
        ok += st == SJHIP_COL_OK ? 1u : 0u;
    }
    (void)block_excl_sum(ok, s_ok, tid, &tot_ok);
    longest = block_max(longest, s_len);
    if (tid == 0) o.tiles_len[blockIdx.x] = longest, o.tiles_ok[blockIdx.x] = tot_ok;
}
// (a single-key call; tiles_ok has been scanned into totals[ORDER_T_ACTIVE], the OK rows)  The rows without a key are parked: the OK
// rows go to the front in row order, the others behind them in row order, where they stay.  Without sort_keys into perm, the OK rows
// active in one class at the positions 0 .. n_ok: the rounds follow.  With sort_keys -- a numeric key, which one sort orders -- as
// the (key, row) pairs of its first pass, the others into both row buffers (whichever the last pass writes, they lie behind it),
// and the tile's AND / OR of the keys for k_q_order_fold
__global__ __launch_bounds__(QT) void k_q_order_park(QOrder o, Arr<u64> sort_keys, Arr<u32> rows0, Arr<u32> rows1) {
    __shared__ unsigned long long s_w[QT / 64], s_k[2][QT / 64];
    const u32 n = o.n, base = blockIdx.x * QTILE + threadIdx.x * QI, n_ok = (u32)o.totals[ORDER_T_ACTIVE];
    const bool direct = sort_keys ? true : false;
    u32 f[QI], sum = 0;
#pragma unroll
    for (int k = 0; k < QI; k++) {
        f[k] = base + k < n && o.status[base + k] == SJHIP_COL_OK ? 1u : 0u;
        sum += f[k];
    }
    u32 at = (u32)(o.tiles_ok[blockIdx.x] + block_excl_sum(sum, s_w, (int)threadIdx.x, nullptr));
    u64 all = ~0ull, any = 0;
#pragma unroll
    for (int k = 0; k < QI; k++) {
        const u32 i = base + k;
        if (i >= n) break;
        const u32 behind = n_ok + (i - at);  // (i - at: the rows without a key in front of row i)
        if (f[k]) {
            if (direct) {
                const u64 key = o.kidx[i];
                sort_keys[at] = key;
                rows0[at] = i;
                all &= key, any |= key;
            } else {
                o.perm[at] = i;
                o.row[at] = i;
                o.pos[at] = at;
                o.cls[at] = 1;
            }
            at++;
        } else if (direct) rows0[behind] = i, rows1[behind] = i;
        else o.perm[behind] = i;
    }
    if (!direct) return;
    block_and_or(all, any, s_k);
    if (threadIdx.x == 0) {
        o.tiles_kand[blockIdx.x] = all, o.tiles_kor[blockIdx.x] = any;
        o.tiles_cand[blockIdx.x] = ~0ull, o.tiles_cor[blockIdx.x] = 0;
    }
}
// at: the byte the round's chunks of a string column begin at; the first input of the sort
__global__ __launch_bounds__(QT) void k_q_order_chunks(QView q, QOrder o, int kind, u32 desc, const unsigned long long *active, u64 at,
                                                      Arr<u64> sort_keys, Arr<u32> sort_rows) {
    __shared__ unsigned long long s_k[2][QT / 64], s_c[2][QT / 64];
    const int tid = threadIdx.x;
    const u32 m = (u32)*active;
    u64 kall = ~0ull, kany = 0, call = ~0ull, cany = 0;
#pragma unroll 1
    for (int k = 0; k < QI; k++) {
        const u32 i = blockIdx.x * QTILE + k * QT + tid;
        if (i >= m) break;
        const u32 r = o.row[i];
        const bool missing = o.status[r] != SJHIP_COL_OK;
        u64 key = 0;
        if (!missing) {
            key = o.kidx[r];
            if (kind == SJHIP_COL_STRING) {
                const u64 w = q.tape[key], len = q.tape[key + 1];
                key = strord_chunk(str_bytes(q, w, len), len, at);
                if (desc) key = ~key;
            }
            kall &= key, kany |= key;
        }
        const u32 c = mkord_class_key(o.cls[i], missing);
        o.chunk[i] = key;
        o.ckey[i] = c;
        sort_keys[i] = key;
        sort_rows[i] = i;
        call &= c, cany |= c;
    }
    block_and_or(kall, kany, s_k);
    block_and_or(call, cany, s_c);
    if (tid == 0) {
        o.tiles_kand[blockIdx.x] = kall, o.tiles_kor[blockIdx.x] = kany;
        o.tiles_cand[blockIdx.x] = call, o.tiles_cor[blockIdx.x] = cany;
    }
}
// one block: the ANDs and ORs over the tiles of k_q_order_chunks (a tile without an entry holds the identities); key_tiles > 0: the
// longest key over the tiles of k_q_order_keys as well
__global__ __launch_bounds__(QT) void k_q_order_fold(QOrder o, u32 tiles, u32 key_tiles) {
    __shared__ unsigned long long s_k[2][QT / 64], s_c[2][QT / 64], s_len[QT / 64];
    u64 kall = ~0ull, kany = 0, call = ~0ull, cany = 0, longest = 0;
    for (u32 t = threadIdx.x; t < tiles; t += QT) {
        kall &= o.tiles_kand[t], kany |= o.tiles_kor[t];
        call &= o.tiles_cand[t], cany |= o.tiles_cor[t];
    }
    for (u32 t = threadIdx.x; t < key_tiles; t += QT) longest = o.tiles_len[t] > longest ? o.tiles_len[t] : longest;
    block_and_or(kall, kany, s_k);
    block_and_or(call, cany, s_c);
    longest = block_max(longest, s_len);
    if (threadIdx.x == 0) {
        o.totals[ORDER_T_ANDOR] = kall, o.totals[ORDER_T_ANDOR + 1] = kany;
        o.totals[ORDER_T_ANDOR + 2] = call, o.totals[ORDER_T_ANDOR + 3] = cany;
        if (key_tiles) o.totals[ORDER_T_LONGEST] = longest;
    }
}
// sorted: the active entries ordered by chunk key; ckey: their class keys -> the input of the sort by class key
__global__ __launch_bounds__(256) void k_q_order_classes(Arr<const u32> ckey, u32 m, Arr<const u32> sorted, Arr<u32> sort_keys, Arr<u32> sort_rows) {
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const u32 e = sorted[i];
    sort_keys[i] = ckey[e];
    sort_rows[i] = e;
}
// sorted: the m active entries ordered by (class key, chunk key).  A thread takes QI consecutive ones and looks at both neighbours
__global__ __launch_bounds__(QT) void k_q_order_place(QOrder o, u32 m, Arr<const u32> sorted, u32 is_string, u32 desc) {
    __shared__ unsigned long long s_w[QT / 64];
    const u32 base = blockIdx.x * QTILE + threadIdx.x * QI;
    u32 e[QI + 2], c[QI + 2];
    u64 key[QI + 2];
    bool in[QI + 2];
#pragma unroll
    for (int k = 0; k < QI + 2; k++) {
        const u32 i = base + (u32)k - 1u;  // (base = 0, k = 0: wraps beyond m)
        in[k] = i < m;
        e[k] = in[k] ? sorted[i] : 0u;
        c[k] = in[k] ? o.ckey[e[k]] : 0u;
        key[k] = in[k] ? o.chunk[e[k]] : 0ull;
    }
    unsigned long long heads = 0, active = 0, tot_h = 0, tot_a = 0;
#pragma unroll
    for (int k = 1; k <= QI; k++) {
        if (!in[k]) break;
        const bool head = !in[k - 1] || c[k] != c[k - 1] || key[k] != key[k - 1];
        const bool next_head = !in[k + 1] || c[k + 1] != c[k] || key[k + 1] != key[k];
        const bool full = is_string && strord_chunk_count(key[k], desc != 0) == (u32)STRORD_CHUNK;
        const bool stays = mkord_stays((c[k] & 1u) != 0, head && next_head, full);
        const u32 i = base + (u32)k - 1u, p = o.pos[i];
        o.perm[p] = o.row[e[k]];
        if (head) o.bnd[p] = 1;
        o.flags[i] = (u8)((head ? 1u : 0u) | (stays ? 2u : 0u));
        heads += head ? 1u : 0u;
        active += stays ? 1u : 0u;
    }
    (void)block_excl_sum(heads, s_w, (int)threadIdx.x, &tot_h);
    (void)block_excl_sum(active, s_w, (int)threadIdx.x, &tot_a);
    if (threadIdx.x == 0) o.tiles_head[blockIdx.x] = tot_h, o.tiles_act[blockIdx.x] = tot_a;
}
// (tiles_head and tiles_act have been scanned)  The entries that stay active, in position order, into the next round's arrays: the row, the
// position it was placed at, and its new class -- the heads up to and including it
__global__ __launch_bounds__(QT) void k_q_order_compact(QOrder o, u32 m, Arr<const u32> sorted) {
    __shared__ unsigned long long s_w[QT / 64];
    const u32 base = blockIdx.x * QTILE + threadIdx.x * QI;
    u32 f[QI], heads = 0, active = 0;
#pragma unroll
    for (int k = 0; k < QI; k++) {
        f[k] = base + k < m ? o.flags[base + k] : 0u;
        heads += f[k] & 1u;
        active += f[k] >> 1;
    }
    u32 cl = (u32)(o.tiles_head[blockIdx.x] + block_excl_sum(heads, s_w, (int)threadIdx.x, nullptr));
    u32 at = (u32)(o.tiles_act[blockIdx.x] + block_excl_sum(active, s_w, (int)threadIdx.x, nullptr));
#pragma unroll
    for (int k = 0; k < QI; k++) {
        const u32 i = base + k;
        cl += f[k] & 1u;
        if (f[k] & 2u) {
            o.row_out[at] = o.row[sorted[i]];
            o.pos_out[at] = o.pos[i];
            o.cls_out[at] = cl;
            at++;
        }
    }
}
// b: bnd at the thread's QI positions from `base` and at the one behind them (1 beyond n); of its positions, the classes that begin
// there and those that are not alone in their class
__device__ __forceinline__ void order_bnd_counts(const QOrder &o, u32 base, u32 (&b)[QI + 1], u32 &heads, u32 &active) {
#pragma unroll
    for (int k = 0; k <= QI; k++) b[k] = base + k <= o.n ? o.bnd[base + k] : 1u;
    heads = 0, active = 0;
#pragma unroll
    for (int k = 0; k < QI; k++) {
        if (base + k >= o.n) break;
        heads += b[k];
        active += b[k] && b[k + 1] ? 0u : 1u;
    }
}
// over the n positions: the classes that begin in the tile, and its positions that are not alone in their class
__global__ __launch_bounds__(QT) void k_q_order_bounds(QOrder o) {
    __shared__ unsigned long long s_w[QT / 64];
    u32 b[QI + 1], heads, active;
    order_bnd_counts(o, blockIdx.x * QTILE + threadIdx.x * QI, b, heads, active);
    unsigned long long tot_h = 0, tot_a = 0;
    (void)block_excl_sum(heads, s_w, (int)threadIdx.x, &tot_h);
    (void)block_excl_sum(active, s_w, (int)threadIdx.x, &tot_a);
    if (threadIdx.x == 0) o.tiles_head[blockIdx.x] = tot_h, o.tiles_act[blockIdx.x] = tot_a;
}
// (tiles_head and tiles_act have been scanned)  The next column's active entries, in position order
__global__ __launch_bounds__(QT) void k_q_order_rebuild(QOrder o) {
    __shared__ unsigned long long s_w[QT / 64];
    const u32 n = o.n, base = blockIdx.x * QTILE + threadIdx.x * QI;
    u32 b[QI + 1], heads, active;
    order_bnd_counts(o, base, b, heads, active);
    u32 cl = (u32)(o.tiles_head[blockIdx.x] + block_excl_sum(heads, s_w, (int)threadIdx.x, nullptr));
    u32 at = (u32)(o.tiles_act[blockIdx.x] + block_excl_sum(active, s_w, (int)threadIdx.x, nullptr));
#pragma unroll
    for (int k = 0; k < QI; k++) {
        const u32 p = base + k;
        if (p >= n) break;
        cl += b[k];
        if (!(b[k] && b[k + 1])) {
            o.row[at] = o.perm[p];
            o.pos[at] = p;
            o.cls[at] = cl;
            at++;
        }
    }
}
// rows: the rows in rank order.  One lane per rank: every row is written once
__global__ __launch_bounds__(256) void k_q_order_flag(Arr<const u32> rows, u32 n, u64 limit, Arr<u8> flag) {
    const u32 p = blockIdx.x * 256 + threadIdx.x;
    if (p < n) flag[rows[p]] = p < limit ? 1 : 0;
}
__global__ __launch_bounds__(QT) void k_q_order_flag_sums(Arr<u8> flag, u32 n, unsigned long long *tiles) { tile_sums(arr_raw(flag), n, tiles); }
struct OrderOut {  // the product (d_order), see order_layout
    Arr<u64> order, values;  // [kept]
    Arr<u8> status;          // [kept]
};
// behind the narrowing: order[p] = pre[row(p)], the row's number in the new selection, and its status.  keys: null, or the sort
// keys of the rows' numbers of `kind` (desc: complemented) -> values[p], 0 where the status is not OK
__global__ __launch_bounds__(256) void k_q_order_emit(Arr<const u32> rows, Arr<const u8> status, Arr<const u64> keys, int kind, u32 desc,
                                                      Arr<const u32> pre, u32 kept, OrderOut out) {
    const u32 p = blockIdx.x * 256 + threadIdx.x;
    if (p >= kept) return;
    const u32 row = rows[p];
    const u8 st = status[row];
    out.order[p] = pre[row];
    out.status[p] = st;
    if (keys) {
        const u64 key = keys[row];
        out.values[p] = st == SJHIP_COL_OK ? agg_unkey(desc ? ~key : key, kind) : 0ull;
    }
}

}  // namespace

namespace sj {
// nl_off and the record count of the last stage-2 run in this workspace (stage2.hip)
void stage2_records_view(void *ws, size_t n_tokens, const uint32_t **nl_off);
}

// debug build (-DSJ_DEBUG_BOUNDS): an out-of-bounds access of a query kernel fails the call (this translation unit's record)
static int query_bounds_check(sjhip_ctx *ctx) {
#if defined(SJ_DEBUG_BOUNDS)
    BoundsHit h;
    if (bounds_take(&h) && h.hits) {
        ctx_set_error(ctx, "bounds check (query): %u out-of-bounds accesses, the first to array %u (sj_bounds.h ArrId) at element %llu of %llu",
                      h.hits, h.id, h.index, h.size);
        return SJHIP_ERR_HIP;
    }
#else
    (void)ctx;
#endif
    return SJHIP_OK;
}

static int no_result(sjhip_ctx *ctx) { return sj::no_result(ctx, "queries follow"); }
static int check_key_value(sjhip_ctx *ctx, const uint8_t *key, size_t klen, const uint8_t *val, size_t vlen) {
    if (!ctx || !key || !val) return SJHIP_ERR_ARG;
    if (klen > QMAX || vlen > QMAX) {
        ctx_set_error(ctx, "query key / value longer than %d bytes", QMAX);
        return SJHIP_ERR_ARG;
    }
    return SJHIP_OK;
}
// view of the result held by `part` (ctx itself, or one shard context of ctx's sharded result) with the key and the value of a
// query (checked by the caller: check_key_value); errors are left in ctx.  on_rows: the query runs on the rows of ctx's row
// selection, if it has one (the filter and countWhere stay on records).
static bool selected(const sjhip_ctx *ctx, bool on_rows) { return on_rows && ctx->res.rows.exists(); }
// the rows of this part: what a path query of ctx runs over -- the part's rows of the selection, or its records
static uint32_t part_rows(const sjhip_ctx *ctx, const sjhip_ctx *part, bool on_rows) {
    return selected(ctx, on_rows) ? (uint32_t)part->res.rows.sizes().rows : part->q_records + 1u;
}
static int make_view(sjhip_ctx *ctx, sjhip_ctx *part, const uint8_t *key, size_t klen, const uint8_t *val, size_t vlen, QView *q,
                     bool on_rows) {
    if (!part->res.resident()) return no_result(ctx);
    const uint32_t *nl = nullptr;
    stage2_records_view(part->d_s2.p, part->p_nlay, &nl);
    // (pointers moved down by the shard's bases: see QView; all zero for an unsharded result)
    const u64 tape_base = part->res.tape_base(), strings_base = part->res.strings_base(), msg_base = part->res.msg_base();
    q->tape_base = tape_base;
    q->tape = SJ_ARR((const u64 *)part->d_tape.p - tape_base, tape_base + part->tape_len, A_TAPE);
    q->tape_len = tape_base + part->tape_len;
    q->strings = SJ_ARR((const u8 *)part->d_strings.p - strings_base, strings_base + part->strings_len, A_STRINGS);
    q->strings_len = part->strings_len;
    q->msg = SJ_ARR((const u8 *)part->p_msg - msg_base, msg_base + part->p_len, A_MSG);
    q->msg_len = part->p_len;
    q->nl_off = SJ_ARR(nl, part->q_records, A_NL_OFF);
    q->R = part->q_records;
    q->rows = nullptr;
    q->n_rows = 0;
    if (selected(ctx, on_rows)) {
        const ResultState::Rows &z = part->res.rows.sizes();
        RowsOut o;
        (void)rows_layout(Carve(part->d_rows.p), z.records, z.rows, &o);
        q->rows = SJ_ARR((const u64 *)o.index, z.rows, A_ROWS);
        q->n_rows = z.rows;
    }
    memset(q->key, 0, QMAX);
    memset(q->val, 0, QMAX);
    memcpy(q->key, key, klen);
    memcpy(q->val, val, vlen);
    q->klen = (u32)klen;
    q->vlen = (u32)vlen;
    return SJHIP_OK;
}

// Every part of ctx's result (sj_ctx.h result_parts): Iter / ForEach / FindElement of the reference work on any ParsedJson
// (parsed_json.go:96,125,833); here the queries run part by part in the merged index space (QView) and the host adds the counts
// up / lays the per-record answers end to end.  enqueue(k, part) queues the work of part k on the part's stream (its device is
// current); when every part has been queued -- so the shards on different devices overlap -- each is waited for and collect(k, part)
// reads what came back.  `sync`: the name of the wait in an error.
template <typename E, typename C>
static int walk_parts(sjhip_ctx *ctx, const std::vector<sjhip_ctx *> &parts, const char *sync, E enqueue, C collect) {
    for (size_t k = 0; k < parts.size(); k++) {
        HIPCHK(hipSetDevice(parts[k]->device), "hipSetDevice");
        const int rc = enqueue(k, parts[k]);
        if (rc) return rc;
    }
    for (size_t k = 0; k < parts.size(); k++) {
        HIPCHK(hipSetDevice(parts[k]->device), "hipSetDevice");
        HIPCHK(hipStreamSynchronize(parts[k]->stream), sync);
        collect(k, parts[k]);
    }
    HIPCHK(hipSetDevice(ctx->device), "hipSetDevice");
    return SJHIP_OK;
}
// The parts of a query with a key (or the keys of a path) and a value; an error if there is nothing to ask.
static int query_parts(sjhip_ctx *ctx, const uint8_t *key, size_t klen, const uint8_t *val, size_t vlen, std::vector<sjhip_ctx *> *parts) {
    const int rc = check_key_value(ctx, key, klen, val, vlen);
    if (rc) return rc;
    *parts = result_parts(ctx);
    return parts->empty() ? no_result(ctx) : SJHIP_OK;
}
// ... and the walk of a query kernel over them: enqueue(k, part, q, n) gets the part's view, its n rows (part_rows) and
// kat_bytes(part, n) bytes of the part's d_kat; a part without rows is passed over -- nothing is launched for it (a grid of 0
// blocks is a launch error), collect(k, part) still runs.  The bounds check of the debug build follows the last wait.
template <typename K, typename E, typename C>
static int query_over_parts(sjhip_ctx *ctx, const std::vector<sjhip_ctx *> &parts, const uint8_t *key, size_t klen, const uint8_t *val,
                            size_t vlen, bool on_rows, const char *sync, K kat_bytes, E enqueue, C collect) {
    const int rc = walk_parts(ctx, parts, sync, [&](size_t k, sjhip_ctx *part) -> int {
        QView q;
        int rc = make_view(ctx, part, key, klen, val, vlen, &q, on_rows);
        if (rc) return rc;
        const uint32_t n = part_rows(ctx, part, on_rows);
        if (n == 0) return SJHIP_OK;
        rc = arena_reserve(part, part->d_kat, kat_bytes(part, n));
        return rc ? rc : enqueue(k, part, q, n);
    }, collect);
    return rc ? rc : query_bounds_check(ctx);
}
static const uint8_t NO_VALUE = 0;  // the value of a query that has none (vlen 0)

// Runs `launch(part, q, n, d_count)` on every part of ctx's result and adds the 8-byte counts up.
template <typename F>
static int count_over_parts(sjhip_ctx *ctx, const uint8_t *key, size_t klen, const uint8_t *val, size_t vlen, bool on_rows, uint64_t *count,
                            F launch) {
    std::vector<sjhip_ctx *> parts;
    const int rc = query_parts(ctx, key, klen, val, vlen, &parts);
    if (rc) return rc;
    uint64_t total = 0;
    for (sjhip_ctx *part : parts) *(unsigned long long *)(part->h_scratch + 512) = 0;  // (a part without rows copies nothing back)
    const int rc2 = query_over_parts(ctx, parts, key, klen, val, vlen, on_rows, "count sync", [](const sjhip_ctx *, uint32_t) { return (size_t)64; },
        [&](size_t, sjhip_ctx *part, const QView &q, uint32_t n) -> int {
            HIPCHK(hipMemsetAsync(part->d_kat.p, 0, 8, part->stream), "count memset");
            launch(part, q, n, (unsigned long long *)part->d_kat.p);
            HIPCHK(hipGetLastError(), "count launch");
            HIPCHK(hipMemcpyAsync(part->h_scratch + 512, part->d_kat.p, 8, hipMemcpyDeviceToHost, part->stream), "D2H count");
            return SJHIP_OK;
        },
        [&](size_t, sjhip_ctx *part) { total += *(const unsigned long long *)(part->h_scratch + 512); });
    if (rc2 == SJHIP_OK) *count = total;
    return rc2;
}

// countWhere(key, value) is the path count with one key: the first member with the key wins, top level only, and its value must
// be a string equal to `value` after unescaping
static QPath one_key_path(size_t klen) {
    QPath pth;
    for (u32 &e : pth.end) e = (u32)klen;
    pth.n = 1;
    return pth;
}
int sjhip_count_where(sjhip_ctx *ctx, const uint8_t *key, size_t klen, const uint8_t *value, size_t vlen, uint64_t *count) {
    if (!count) return SJHIP_ERR_ARG;
    const QPath pth = one_key_path(klen);
    return count_over_parts(ctx, key, klen, value, vlen, false, count, [&](sjhip_ctx *part, const QView &q, uint32_t n, unsigned long long *d) {
        hipLaunchKernelGGL(k_q_count_path, dim3((n + 255) / 256), dim3(256), 0, part->stream, q, pth, (int)SJHIP_OP_EQ_STRING, (u64)0, d);
    });
}

int sjhip_filter_where(sjhip_ctx *ctx, const uint8_t *key, size_t klen, const uint8_t *value, size_t vlen,
                       uint64_t *n_records, size_t *tape_len, size_t *strings_len) {
    if (ctx && !ctx->res.whole()) return no_whole_result(ctx, "sjhip_filter_where", "queries follow");  // the unsharded result of ctx itself
    QView q;
    int rc = check_key_value(ctx, key, klen, value, vlen);
    if (rc == SJHIP_OK) rc = make_view(ctx, ctx, key, klen, value, vlen, &q, false);
    if (rc) return rc;
    const uint32_t n = ctx->q_records + 1u;
    if (!(ctx->p_flags & SJHIP_FLAG_COPY_STRINGS)) {
        ctx_set_error(ctx, "sjhip_filter_where needs a parse with SJHIP_FLAG_COPY_STRINGS (the filtered Strings.B is self-contained)");
        return SJHIP_ERR_ARG;
    }
    HIPCHK(hipSetDevice(ctx->device), "hipSetDevice");
    ctx->res.claim_shared();
    const u32 tiles = (n + QTILE - 1) / QTILE;
    QRec o;
    QTiles T;
    auto layout = [&](Carve c) {
        o.totals = c.take<unsigned long long>(32);
        o.flag = c.take<u32>(n);
        o.words = c.take<u32>(n);
        o.first_str = c.take<u32>(n);
        o.s_len = c.take<u32>(n);
        o.s_pre = c.take<u32>(n);
        T.tw = c.take<unsigned long long>(tiles);
        T.tb = c.take<unsigned long long>(tiles);
        T.tc = c.take<unsigned long long>(tiles);
        T.tf = c.take<long long>(tiles);
        return c.used;
    };
    rc = arena_reserve(ctx, ctx->d_q, layout(Carve()));
    if (rc) return rc;
    rc = arena_reserve(ctx, ctx->d_qtape, ctx->tape_len * 8 + 64);
    if (rc) return rc;
    rc = arena_reserve(ctx, ctx->d_qstrings, ctx->strings_len + 64);
    if (rc) return rc;
    (void)layout(Carve(ctx->d_q.p));
    unsigned long long *const none = nullptr;
    hipLaunchKernelGGL(k_q_mark, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, q, one_key_path(klen), o);
    hipLaunchKernelGGL(k_q_tile_sums, dim3(tiles), dim3(QT), 0, ctx->stream, o, n, T);
    hipLaunchKernelGGL(k_tw_scan_sums, dim3(1), dim3(1024), 0, ctx->stream, T.tc, T.tw, none, tiles, o.totals);
    hipLaunchKernelGGL(k_tw_scan_last, dim3(1), dim3(1024), 0, ctx->stream, T.tf, tiles);
    hipLaunchKernelGGL(k_q_tile_apply1, dim3(tiles), dim3(QT), 0, ctx->stream, o, n, T, (u32)q.strings_len);
    hipLaunchKernelGGL(k_tw_scan_sums, dim3(1), dim3(1024), 0, ctx->stream, none, none, T.tb, tiles, o.totals);
    hipLaunchKernelGGL(k_q_tile_apply2, dim3(tiles), dim3(QT), 0, ctx->stream, o, n, T);
    HIPCHK(hipGetLastError(), "filter launch");
    unsigned long long *h = (unsigned long long *)(ctx->h_scratch + 512);
    HIPCHK(hipMemcpyAsync(h, o.totals, 24, hipMemcpyDeviceToHost, ctx->stream), "D2H totals");
    HIPCHK(hipStreamSynchronize(ctx->stream), "filter sync");
    rc = published(ctx, ctx->res.publish_filtered({(size_t)h[1], (size_t)h[2]}));
    if (rc) return rc;
    if (n_records) *n_records = h[0];
    if (tape_len) *tape_len = (size_t)h[1];
    if (strings_len) *strings_len = (size_t)h[2];
    if (h[0] == 0) return query_bounds_check(ctx);
    hipLaunchKernelGGL(k_q_copy, dim3((n + 3) / 4), dim3(256), 0, ctx->stream, q, o, SJ_ARR((u64 *)ctx->d_qtape.p, h[1], A_FROWS_TAPE),
                       SJ_ARR((u8 *)ctx->d_qstrings.p, h[2], A_FROWS_STRINGS));
    HIPCHK(hipGetLastError(), "filter copy launch");
    return SJHIP_OK;
}

int sjhip_fetch_filtered(sjhip_ctx *ctx, uint64_t *tape_dst, uint8_t *strings_dst) {
    if (!ctx) return SJHIP_ERR_ARG;
    if (!ctx->res.filtered()) {  // no filter ran, or a later parse / serialize / marshal call re-used its arenas
        ctx_set_error(ctx, "no filtered result on the device (sjhip_fetch_filtered follows sjhip_filter_where or sjhip_filter_rows)");
        return SJHIP_ERR_ARG;
    }
    HIPCHK(hipSetDevice(ctx->device), "hipSetDevice");
    const ResultState::Filtered &f = ctx->res.filtered_sizes();
    if (f.tape_len && tape_dst)
        HIPCHK(hipMemcpyAsync(tape_dst, ctx->d_qtape.p, f.tape_len * 8, hipMemcpyDeviceToHost, ctx->stream), "D2H filtered tape");
    if (f.strings_len && strings_dst)
        HIPCHK(hipMemcpyAsync(strings_dst, ctx->d_qstrings.p, f.strings_len, hipMemcpyDeviceToHost, ctx->stream),
               "D2H filtered strings");
    HIPCHK(hipStreamSynchronize(ctx->stream), "fetch sync");
    return query_bounds_check(ctx);  // (debug build: the copy kernel of sjhip_filter_where / sjhip_filter_rows has finished here)
}

// ---- paths, typed values, key sets ------------------------------------------------------------------------------------------
// the keys of a path / key set: where each one ends in the concatenation (QView::key holds the bytes)
// (may_be_empty: sjhip_select_rows alone takes a path of no keys -- the array is the root value -- and then no key arrays)
static int make_path(sjhip_ctx *ctx, const uint8_t *keys, const uint32_t *key_lens, uint32_t n_keys, QPath *pth, size_t *total_out,
                     bool may_be_empty = false) {
    if (!ctx || ((!keys || !key_lens) && n_keys) || (n_keys == 0 && !may_be_empty)) return SJHIP_ERR_ARG;
    if (n_keys > (uint32_t)QPATH_MAX) {
        ctx_set_error(ctx, "a path / key set holds at most %d keys", QPATH_MAX);
        return SJHIP_ERR_ARG;
    }
    size_t total = 0;
    for (uint32_t j = 0; j < n_keys; j++) {
        total += key_lens[j];
        if (total > (size_t)QMAX) {
            ctx_set_error(ctx, "the keys of a path / key set are longer than %d bytes together", QMAX);
            return SJHIP_ERR_ARG;
        }
        pth->end[j] = (u32)total;
    }
    for (uint32_t j = n_keys; j < (uint32_t)QPATH_MAX; j++) pth->end[j] = (u32)total;
    pth->n = n_keys;
    *total_out = total;
    return SJHIP_OK;
}

// Per-record answers of every part of ctx's result -- per row, under a row selection: `records` count rows then -- laid end to
// end in document order: output k holds outs[k].width bytes for every record at outs[k].dst; launch(part, q, n, d) fills n records of every output, output k at d[k] on the part's device.
// cap_records: room in the outputs; *records: records of the whole result.
struct RecOut {
    void *dst;
    uint32_t width;  // bytes per record
};
static constexpr int MAX_OUTS = 2;
template <typename F>
static int outputs_over_parts(sjhip_ctx *ctx, const uint8_t *keys, size_t klen, const RecOut *outs, int n_outs, size_t cap_records,
                              size_t *records, const char *who, F launch) {
    std::vector<sjhip_ctx *> parts;
    const int rc = query_parts(ctx, keys, klen, &NO_VALUE, 0, &parts);
    if (rc) return rc;
    size_t total = 0;
    for (sjhip_ctx *part : parts) total += part_rows(ctx, part, true);
    *records = total;
    if (cap_records < total) {
        ctx_set_error(ctx, "%s: room for %zu records, the result holds %zu", who, cap_records, total);
        return SJHIP_ERR_ARG;
    }
    auto layout = [&](Carve c, uint32_t n, u8 **d) {
        for (int j = 0; j < n_outs; j++) d[j] = c.take<u8>((size_t)n * outs[j].width);
        return c.used;
    };
    size_t at = 0;
    return query_over_parts(ctx, parts, keys, klen, &NO_VALUE, 0, true, "query sync",
        [&](const sjhip_ctx *, uint32_t n) {
            u8 *d[MAX_OUTS];
            return layout(Carve(), n, d) + 64;
        },
        [&](size_t, sjhip_ctx *part, const QView &q, uint32_t n) -> int {
            u8 *d[MAX_OUTS];
            (void)layout(Carve(part->d_kat.p), n, d);
            launch(part, q, n, d);
            HIPCHK(hipGetLastError(), "query launch");
            for (int j = 0; j < n_outs; j++)
                HIPCHK(hipMemcpyAsync((u8 *)outs[j].dst + at * outs[j].width, d[j], (size_t)n * outs[j].width, hipMemcpyDeviceToHost,
                                      part->stream), "D2H per-record answers");
            at += n;
            return SJHIP_OK;
        },
        [](size_t, sjhip_ctx *) {});
}
// `per` 8-byte words for every record in `out`
template <typename F>
static int records_over_parts(sjhip_ctx *ctx, const uint8_t *keys, size_t klen, uint32_t per, uint64_t *out, size_t cap_records,
                              size_t *records, const char *who, F launch) {
    const RecOut o = {out, per * 8u};
    return outputs_over_parts(ctx, keys, klen, &o, 1, cap_records, records, who,
                              [&](sjhip_ctx *part, const QView &q, uint32_t n, u8 *const *d) { launch(part, q, n, (u64 *)d[0]); });
}

int sjhip_find_path(sjhip_ctx *ctx, const uint8_t *keys, const uint32_t *key_lens, uint32_t n_keys, uint64_t *index_out,
                    size_t cap, size_t *records) {
    if (!index_out || !records) return SJHIP_ERR_ARG;
    QPath pth;
    size_t klen = 0;
    const int rc = make_path(ctx, keys, key_lens, n_keys, &pth, &klen);
    if (rc) return rc;
    return records_over_parts(ctx, keys, klen, 1, index_out, cap, records, "sjhip_find_path",
                              [&](sjhip_ctx *part, const QView &q, uint32_t n, u64 *d) {
                                  hipLaunchKernelGGL(k_q_find_path, dim3((n + 255) / 256), dim3(256), 0, part->stream, q, pth, d);
                              });
}

// The value of a typed predicate (sjhip_count_where_path, sjhip_where_path): a number -- an int64_t, uint64_t or double, 8 bytes --
// or a bool (1 byte) travels as *want; a string (EQ_STRING, PREFIX_STRING) travels in the view.  An unknown operator, or a value
// of another size: SJHIP_ERR_ARG.
static int predicate_value(int op, const void *value, size_t vlen, u64 *want, bool *is_str) {
    if (op < SJHIP_OP_EXISTS || op > SJHIP_OP_PREFIX_STRING) return SJHIP_ERR_ARG;
    *is_str = op == SJHIP_OP_EQ_STRING || op == SJHIP_OP_PREFIX_STRING;
    *want = 0;
    if ((op >= SJHIP_OP_EQ_INT && op <= SJHIP_OP_EQ_FLOAT) || (op >= SJHIP_OP_LT_INT && op <= SJHIP_OP_GE_FLOAT)) {
        if (!value || vlen != 8) return SJHIP_ERR_ARG;
        memcpy(want, value, 8);
    } else if (op == SJHIP_OP_EQ_BOOL) {
        if (!value || vlen != 1) return SJHIP_ERR_ARG;
        *want = *(const uint8_t *)value != 0;
    } else if (*is_str && !value && vlen) {
        return SJHIP_ERR_ARG;
    }
    return SJHIP_OK;
}
int sjhip_count_where_path(sjhip_ctx *ctx, const uint8_t *keys, const uint32_t *key_lens, uint32_t n_keys, int op,
                           const void *value, size_t vlen, uint64_t *count) {
    if (!count) return SJHIP_ERR_ARG;
    bool is_str = false;
    u64 want = 0;
    int rc = predicate_value(op, value, vlen, &want, &is_str);
    if (rc) return rc;
    QPath pth;
    size_t klen = 0;
    rc = make_path(ctx, keys, key_lens, n_keys, &pth, &klen);
    if (rc) return rc;
    return count_over_parts(ctx, keys, klen, is_str && value ? (const uint8_t *)value : &NO_VALUE, is_str ? vlen : 0, true, count,
                            [&](sjhip_ctx *part, const QView &q, uint32_t n, unsigned long long *d) {
                                hipLaunchKernelGGL(k_q_count_path, dim3((n + 255) / 256), dim3(256), 0, part->stream, q, pth, op, want, d);
                            });
}

int sjhip_project_keys(sjhip_ctx *ctx, const uint8_t *keys, const uint32_t *key_lens, uint32_t n_keys, uint64_t *out,
                       size_t cap_records, size_t *records) {
    if (!out || !records) return SJHIP_ERR_ARG;
    QPath set;
    size_t klen = 0;
    const int rc = make_path(ctx, keys, key_lens, n_keys, &set, &klen);
    if (rc) return rc;
    for (uint32_t a = 0; a < n_keys; a++)  // a set: the reference's onlyKeys is a map
        for (uint32_t b = a + 1; b < n_keys; b++) {
            const u32 ab = a ? set.end[a - 1] : 0, bb = set.end[b - 1];
            if (set.end[a] - ab == set.end[b] - bb && memcmp(keys + ab, keys + bb, set.end[a] - ab) == 0) {
                ctx_set_error(ctx, "sjhip_project_keys: key %u and key %u are equal", a, b);
                return SJHIP_ERR_ARG;
            }
        }
    return records_over_parts(ctx, keys, klen, n_keys, out, cap_records, records, "sjhip_project_keys",
                              [&](sjhip_ctx *part, const QView &q, uint32_t n, u64 *d) {
                                  hipLaunchKernelGGL(k_q_project, dim3((n + 255) / 256), dim3(256), 0, part->stream, q, set, d);
                              });
}

// ---- columns ------------------------------------------------------------------------------------------------------------------
int sjhip_extract_path(sjhip_ctx *ctx, const uint8_t *keys, const uint32_t *key_lens, uint32_t n_keys, int kind, void *values,
                       uint8_t *status, size_t cap_records, size_t *records) {
    if (!values || !status || !records || kind < SJHIP_COL_FLOAT || kind > SJHIP_COL_BOOL) return SJHIP_ERR_ARG;
    QPath pth;
    size_t klen = 0;
    const int rc = make_path(ctx, keys, key_lens, n_keys, &pth, &klen);
    if (rc) return rc;
    const RecOut outs[2] = {{values, kind == SJHIP_COL_BOOL ? 1u : 8u}, {status, 1u}};
    return outputs_over_parts(ctx, keys, klen, outs, 2, cap_records, records, "sjhip_extract_path",
                              [&](sjhip_ctx *part, const QView &q, uint32_t n, u8 *const *d) {
                                  hipLaunchKernelGGL(k_q_extract, dim3((n + 255) / 256), dim3(256), 0, part->stream, q, pth, kind,
                                                     (void *)d[0], d[1]);
                              });
}

// ---- aggregates ---------------------------------------------------------------------------------------------------------------
// Both calls are one walk of the parts: per part the work arrays in d_kat (the results first, so that one copy brings back what
// the caller asked for), the heads, the tile kernel and the folds; nothing of the context's result, its products or its
// selection is written.  The total runs as one segment whose `record` 0 holds the answer; the host joins the parts in part order.
struct AggWork {
    u64 *out;                       // [6 * records (+ 6: the histogram of the total)]
    u32 *head;                      // [rows]
    std::vector<AggItem *> items;   // per level (AGG_OWN: none)
    std::vector<u32> tiles;         // tiles of every level: rows -> AGG_TILE per tile -> two items per tile -> ...
};
// (own_out false: the results lie elsewhere -- the grouping's are part of its product -- and the caller sets w->out)
static size_t agg_layout(Carve c, uint32_t n, size_t records, u32 mode, AggWork *w, bool own_out = true) {
    const bool hist = mode == AGG_ONE, heads = mode == AGG_OFFS;
    w->out = own_out ? c.take<u64>(6 * records + (hist ? 6 : 0)) : nullptr;
    w->head = heads ? c.take<u32>(n) : nullptr;
    w->items.clear();
    w->tiles.clear();
    for (u32 m = n;;) {
        const u32 tiles = (m + AGG_TILE - 1) / AGG_TILE;
        w->tiles.push_back(tiles);
        if (mode == AGG_OWN) {  // every row is stored as it is: no items, no folds
            w->items.push_back(nullptr);
            break;
        }
        w->items.push_back(c.take<AggItem>(2 * (size_t)tiles));
        if (tiles == 1) break;
        m = 2 * tiles;
    }
    return c.used;
}
// the kernels of one part: n rows (> 0), `records` result slots; off: the row offsets of the selection (AGG_OFFS)
// (perm: the grouping's row order -- position r of the n is row perm[r] of the view, `off` counts positions; null: position = row)
static int agg_enqueue(sjhip_ctx *ctx, sjhip_ctx *part, const QView &q, const QPath &pth, int kind, u32 mode, uint32_t n, size_t records,
                       const u64 *off, const AggWork &w, const u32 *perm = nullptr) {
    QAgg a;
    a.kind = kind;
    a.mode = mode;
    a.perm = SJ_ARR(perm, perm ? n : 0, A_SORT);
    a.n_perm = n;
    a.head = SJ_ARR((const u32 *)w.head, n, A_AGG_HEAD);
    a.out = SJ_ARR(w.out, 6 * records, A_AGG_OUT);
    a.records = records;
    a.hist = mode == AGG_ONE ? (unsigned long long *)(w.out + 6) : nullptr;
    if (mode != AGG_OWN) HIPCHK(hipMemsetAsync(w.out, 0, (6 * records + (a.hist ? 6 : 0)) * 8, part->stream), "aggregate results memset");
    if (mode == AGG_OFFS) {
        HIPCHK(hipMemsetAsync(w.head, 0, (size_t)n * 4, part->stream), "aggregate heads memset");
        hipLaunchKernelGGL(k_q_agg_heads, dim3(((u32)records + 255) / 256), dim3(256), 0, part->stream, SJ_ARR(off, records + 1, A_WHERE_OFF),
                           (u32)records, SJ_ARR(w.head, n, A_AGG_HEAD));
    }
    AggItem *level = w.items[0];
    a.items = SJ_ARR(level, level ? 2 * (size_t)w.tiles[0] : 0, A_AGG_ITEMS);
    hipLaunchKernelGGL(k_q_agg_rows, dim3(w.tiles[0]), dim3(AGG_TILE), 0, part->stream, q, pth, a);
    a.hist = nullptr;
    for (size_t l = 1; mode != AGG_OWN && l < w.tiles.size(); l++) {
        const u32 m = 2 * w.tiles[l - 1];
        const AggItem *const below = level;
        level = w.items[l];
        a.items = SJ_ARR(level, 2 * (size_t)w.tiles[l], A_AGG_ITEMS);
        hipLaunchKernelGGL(k_q_agg_fold, dim3(w.tiles[l]), dim3(AGG_TILE), 0, part->stream, a, SJ_ARR(below, m, A_AGG_ITEMS), m);
    }
    HIPCHK(hipGetLastError(), "aggregate launch");
    return SJHIP_OK;
}
static int agg_args(sjhip_ctx *ctx, const char *who, const uint8_t *keys, const uint32_t *key_lens, uint32_t n_keys, int kind, QPath *pth,
                    size_t *klen, std::vector<sjhip_ctx *> *parts) {
    if (!ctx) return SJHIP_ERR_ARG;
    if (kind != SJHIP_COL_FLOAT && kind != SJHIP_COL_INT && kind != SJHIP_COL_UINT) {
        ctx_set_error(ctx, "%s: kind %d is not SJHIP_COL_FLOAT, SJHIP_COL_INT or SJHIP_COL_UINT", who, kind);
        return SJHIP_ERR_ARG;
    }
    const int rc = make_path(ctx, keys, key_lens, n_keys, pth, klen, true);
    return rc ? rc : query_parts(ctx, keys ? keys : &NO_VALUE, *klen, &NO_VALUE, 0, parts);
}
// unsigned order of the keys = the order of the kind (the device's agg_key, sj_order.h)
static u64 agg_host_key(u64 x, int kind) { return agg_key(x, kind); }

int sjhip_aggregate_path(sjhip_ctx *ctx, const uint8_t *keys, const uint32_t *key_lens, uint32_t n_keys, int kind, sjhip_agg *out) {
    QPath pth;
    size_t klen = 0;
    std::vector<sjhip_ctx *> parts;
    int rc = agg_args(ctx, "sjhip_aggregate_path", keys, key_lens, n_keys, kind, &pth, &klen, &parts);
    if (rc) return rc;
    if (!out) return SJHIP_ERR_ARG;
    const uint8_t *const kb = keys ? keys : &NO_VALUE;
    rc = query_over_parts(ctx, parts, kb, klen, &NO_VALUE, 0, true, "aggregate sync",
        [&](const sjhip_ctx *, uint32_t n) {
            AggWork w;
            return agg_layout(Carve(), n, 1, AGG_ONE, &w) + 64;
        },
        [&](size_t, sjhip_ctx *part, const QView &q, uint32_t n) -> int {
            AggWork w;
            (void)agg_layout(Carve(part->d_kat.p), n, 1, AGG_ONE, &w);
            const int rc = agg_enqueue(ctx, part, q, pth, kind, AGG_ONE, n, 1, nullptr, w);
            if (rc) return rc;
            HIPCHK(hipMemcpyAsync(part->h_scratch + 512, w.out, 12 * 8, hipMemcpyDeviceToHost, part->stream), "D2H aggregate");
            return SJHIP_OK;
        },
        [](size_t, sjhip_ctx *) {});
    if (rc) return rc;
    sjhip_agg t;
    memset(&t, 0, sizeof t);
    bool any = false;
    for (sjhip_ctx *part : parts) {  // in part order: the float sum is added up in it
        const uint32_t n = part_rows(ctx, part, true);
        if (n == 0) continue;  // (nothing was launched, nothing came back)
        const u64 *h = (const u64 *)(part->h_scratch + 512);  // count, not_ok, sum, sum_hi, min, max, status[6]
        t.rows += n;
        for (int k = 0; k < 6; k++) t.status[k] += h[6 + k];
        if (h[0] == 0) continue;
        if (kind == SJHIP_COL_FLOAT) {
            double a, b;
            memcpy(&a, &t.sum_lo, 8);
            memcpy(&b, &h[2], 8);
            a = any ? a + b : b;
            memcpy(&t.sum_lo, &a, 8);
        } else {
            const u64 lo = t.sum_lo + h[2];
            t.sum_hi += h[3] + (lo < t.sum_lo ? 1u : 0u);
            t.sum_lo = lo;
        }
        if (!any || agg_host_key(h[4], kind) < agg_host_key(t.min, kind)) t.min = h[4];
        if (!any || agg_host_key(h[5], kind) > agg_host_key(t.max, kind)) t.max = h[5];
        any = true;
    }
    *out = t;
    return SJHIP_OK;
}

int sjhip_aggregate_path_records(sjhip_ctx *ctx, const uint8_t *keys, const uint32_t *key_lens, uint32_t n_keys, int kind, uint64_t *count,
                                 uint64_t *not_ok, void *sum, uint64_t *sum_hi, void *min, void *max, size_t cap_records, size_t *records) {
    QPath pth;
    size_t klen = 0;
    std::vector<sjhip_ctx *> parts;
    int rc = agg_args(ctx, "sjhip_aggregate_path_records", keys, key_lens, n_keys, kind, &pth, &klen, &parts);
    if (rc) return rc;
    if (!records) return SJHIP_ERR_ARG;
    std::vector<size_t> at(parts.size() + 1, 0);  // the records in front of every part
    for (size_t k = 0; k < parts.size(); k++) at[k + 1] = at[k] + parts[k]->q_records + 1u;
    *records = at[parts.size()];
    if (cap_records < *records) {
        ctx_set_error(ctx, "sjhip_aggregate_path_records: room for %zu records, the result holds %zu", cap_records, *records);
        return SJHIP_ERR_ARG;
    }
    const uint8_t *const kb = keys ? keys : &NO_VALUE;
    const bool sel = selected(ctx, true);
    u8 *const dst[6] = {(u8 *)count, (u8 *)not_ok, (u8 *)sum, (u8 *)sum_hi, (u8 *)min, (u8 *)max};
    for (size_t k = 0; k < parts.size(); k++)  // a part without rows launches nothing: its records hold no row
        if (part_rows(ctx, parts[k], true) == 0)
            for (u8 *d : dst)
                if (d) memset(d + at[k] * 8, 0, (at[k + 1] - at[k]) * 8);
    const u32 mode = sel ? AGG_OFFS : AGG_OWN;
    return query_over_parts(ctx, parts, kb, klen, &NO_VALUE, 0, true, "aggregate sync",
        [&](const sjhip_ctx *part, uint32_t n) {
            AggWork w;
            return agg_layout(Carve(), n, (size_t)part->q_records + 1u, mode, &w) + 64;
        },
        [&](size_t k, sjhip_ctx *part, const QView &q, uint32_t n) -> int {
            const size_t recs = (size_t)part->q_records + 1u;
            AggWork w;
            (void)agg_layout(Carve(part->d_kat.p), n, recs, mode, &w);
            RowsOut sel_rows = {nullptr, nullptr, nullptr};
            if (sel) {
                const ResultState::Rows &z = part->res.rows.sizes();
                (void)rows_layout(Carve(part->d_rows.p), z.records, z.rows, &sel_rows);
            }
            const int rc = agg_enqueue(ctx, part, q, pth, kind, mode, n, recs, sel_rows.off, w);
            if (rc) return rc;
            for (int j = 0; j < 6; j++)
                if (dst[j])
                    HIPCHK(hipMemcpyAsync(dst[j] + at[k] * 8, w.out + (size_t)j * recs, recs * 8, hipMemcpyDeviceToHost, part->stream),
                           "D2H per-record aggregates");
            return SJHIP_OK;
        },
        [](size_t, sjhip_ctx *) {});
}

// ---- products: built on the device part by part, fetched later -- the string column, the list column, the table ---------------
// build_product, the same for all three: the last product is given up; pass 1 over the parts measures -- the product's kernels
// leave a length per record in its work arrays in d_kat, scan_lengths turns them into offsets in place, the totals come back
// through h_scratch + 512 --; pass 2 reserves the product's own arena for those sizes and gathers into it (the work arrays stay
// where they are: nothing more of d_kat is asked for); then the out-parameters and the publish.  fetch_joined is the fetch.
static u32 tiles_of(u32 n) { return (n + 1u + QTILE - 1) / QTILE; }  // the scan tiles of a length array: n + 1 entries
// The exclusive scan, in place, of the length array(s) of `a` (a QCol: one; a QList: two), n + 1 entries each: k_tw_scan_sums
// takes the tile sums of up to three arrays in its slots (null: none) and leaves the grand total of slot i in totals[i].
template <typename A>
static void scan_lengths(sjhip_ctx *part, u32 n, void (*sums)(A, u32), void (*apply)(A, u32), const A &a, unsigned long long *slot0,
                         unsigned long long *slot1, unsigned long long *slot2, unsigned long long *totals) {
    const u32 m = n + 1u, tiles = tiles_of(n);
    hipLaunchKernelGGL(sums, dim3(tiles), dim3(QT), 0, part->stream, a, m);
    hipLaunchKernelGGL(k_tw_scan_sums, dim3(1), dim3(1024), 0, part->stream, slot0, slot1, slot2, tiles, totals);
    hipLaunchKernelGGL(apply, dim3(tiles), dim3(QT), 0, part->stream, a, m);
}
// A layout -- a function of a Carve -- run for its size, the arena reserved for it (+ 64), and run again on the arena.
template <typename L>
static int reserve_layout(sjhip_ctx *part, DevBuf &arena, L layout, size_t *bytes = nullptr) {
    const size_t need = layout(Carve());
    const int rc = arena_reserve(part, arena, need + 64);
    if (rc) return rc;
    (void)layout(Carve(arena.p));
    if (bytes) *bytes = need;
    return SJHIP_OK;
}
// What a product P plugs in (ColumnBuild, ListBuild, TableBuild below):
//   Sizes, product, SYNC_*  what it publishes, where in ResultState, the names of its two waits in an error
//   Work, work()            its work arrays of one part (n rows) and their layout in d_kat, the totals of the scans in front
//   measure()               pass 1 on one part: its kernels and scans, then the D2H of its totals to h_scratch + 512
//   sizes_of(), add()       a part's sizes from what came back, and their sum
//   gather()                pass 2 on one part: its arena(s) for those sizes, its gather kernels
//   finish()                what the total holds beyond sums, and the call's out-parameters
// `keys` / `klen`: the keys of its path(s), which travel in the view.  Errors of the HIP calls are left in ctx, the owner.
template <typename P>
static int build_product(sjhip_ctx *ctx, const uint8_t *keys, size_t klen, P &p) {
    (ctx->res.*P::product).begin();  // (the last one is replaced, whatever happens below)
    std::vector<sjhip_ctx *> parts;
    int rc = query_parts(ctx, keys, klen, &NO_VALUE, 0, &parts);
    if (rc) return rc;
    std::vector<typename P::Work> work(parts.size());
    std::vector<typename P::Sizes> sizes(parts.size());
    typename P::Sizes total;
    static const unsigned long long no_totals[4 * TABLE_MAX_COLS] = {};  // what a part without rows measures
    rc = query_over_parts(ctx, parts, keys, klen, &NO_VALUE, 0, true, P::SYNC_MEASURE,
        [&](const sjhip_ctx *part, uint32_t n) {
            typename P::Work w;
            unsigned long long *totals;
            return p.work(Carve(), part, n, &w, &totals) + 64;
        },
        [&](size_t k, sjhip_ctx *part, const QView &q, uint32_t n) -> int {
            unsigned long long *totals;
            const size_t work_bytes = p.work(Carve(part->d_kat.p), part, n, &work[k], &totals);
            return p.measure(ctx, part, q, n, work[k], work_bytes, totals);
        },
        [&](size_t k, sjhip_ctx *part) {
            const size_t n = part_rows(ctx, part, true);
            sizes[k] = p.sizes_of(n, n ? (const unsigned long long *)(part->h_scratch + 512) : no_totals);
            p.add(&total, sizes[k]);
        });
    if (rc) return rc;
    rc = query_over_parts(ctx, parts, keys, klen, &NO_VALUE, 0, true, P::SYNC_GATHER, [](const sjhip_ctx *, uint32_t) { return (size_t)0; },
        [&](size_t k, sjhip_ctx *part, const QView &q, uint32_t n) -> int { return p.gather(ctx, part, q, n, work[k], sizes[k]); },
        [](size_t, sjhip_ctx *) {});
    if (rc) return rc;
    p.finish(&total);
    bool ok = true;  // the sizes: on every part, then joined on a sharded owner
    for (size_t k = 0; k < parts.size(); k++) ok &= parts[k]->res.publish(P::product, sizes[k]);
    if (ctx->res.sharded()) ok &= ctx->res.publish(P::product, total);
    return published(ctx, ok);
}

// The joined fetch.  A product is a few arrays per part (Seg), each as long as one of the part's counts -- its records, elements
// or bytes -- and laid end to end in the caller's destination.  An offset array (`values` names a domain) starts from 0 in every
// part and its last entry is the next part's first: `count` entries of every part travel, those of a later part are moved up by
// what the parts in front hold in the domain of the VALUES (not the one it is indexed by), the terminating entry is that total.
enum Dom { RECORDS, ELEMS, BYTES, N_DOMS, NO_DOM = -1 };
struct Seg {
    void *dst;         // (null -- where the product's null_dst lets it through -- : this array is not wanted)
    size_t width;      // bytes per element
    int by;            // a part holds count[by] elements
    int values;        // an offset array: the domain its values count in; NO_DOM: data
    const char *what;  // the name of its copy in an error
    bool ends = true;  // an offset array: the total of its values lies behind its last entry (false: values that count in a domain
                       // and are moved up like offsets, but one per element and nothing behind them -- the parent of every row)
};
struct PartArrays {  // of one part: its counts, from its published sizes, and where its arrays lie in its arena (segs' order)
    size_t count[N_DOMS] = {};
    const void *src[4] = {};
};
static int no_product(sjhip_ctx *ctx, const char *text) {  // none was built, or a parse (or sjhip_ctx_trim) came after it
    ctx_set_error(ctx, "%s", text);
    return SJHIP_ERR_ARG;
}
// layout(part, count, src) fills a part's PartArrays; null_dst(total): the product's rules about null destinations, given the joined counts.
template <typename L, typename N>
static int fetch_joined(sjhip_ctx *ctx, const char *sync, const Seg *segs, size_t n_segs, L layout, N null_dst) {
    const std::vector<sjhip_ctx *> parts = result_parts(ctx);
    const size_t P = parts.size();
    std::vector<PartArrays> a(P);
    std::vector<std::array<size_t, N_DOMS>> at(P + 1);  // where every part's records, elements and bytes start
    for (size_t k = 0; k < P; k++) {
        layout(parts[k], a[k].count, a[k].src);
        for (int d = 0; d < N_DOMS; d++) at[k + 1][d] = at[k][d] + a[k].count[d];
    }
    int rc = null_dst(at[P].data());
    if (rc) return rc;
    rc = walk_parts(ctx, parts, sync,
        [&](size_t k, sjhip_ctx *part) -> int {
            for (size_t s = 0; s < n_segs; s++) {
                const Seg &g = segs[s];
                const size_t cnt = a[k].count[g.by];
                if (cnt && g.dst)
                    HIPCHK(hipMemcpyAsync((u8 *)g.dst + at[k][g.by] * g.width, a[k].src[s], cnt * g.width, hipMemcpyDeviceToHost, part->stream), g.what);
            }
            return SJHIP_OK;
        },
        [&](size_t k, sjhip_ctx *) {  // the offsets of a later part: from the end of the parts in front of it
            for (size_t s = 0; s < n_segs; s++) {
                const Seg &g = segs[s];
                if (g.values == NO_DOM || !at[k][g.values] || !g.dst) continue;
                for (size_t i = at[k][g.by]; i < at[k + 1][g.by]; i++) ((uint64_t *)g.dst)[i] += at[k][g.values];
            }
        });
    if (rc) return rc;
    for (size_t s = 0; s < n_segs; s++)
        if (segs[s].values != NO_DOM && segs[s].ends && segs[s].dst) ((uint64_t *)segs[s].dst)[at[P][segs[s].by]] = at[P][segs[s].values];
    return SJHIP_OK;
}

// ---- string columns: one QCol each, the single one (sjhip_extract_path_strings) and those of a table ------------------------------
// A QCol -- the work arrays of one string column in d_kat, which only lives for one call -- is filled by k_q_col_len (the single
// column) or by k_q_table_walk (a table's); everything behind the fill is the same: col_scan, col_gather.
static void col_work(Carve &c, uint32_t n, QCol *col) {
    col->idx = c.take<u64>(n);
    col->off = c.take<u64>((size_t)n + 1);
    col->status = c.take<u8>(n);
    col->tiles = c.take<unsigned long long>(tiles_of(n));
}
static void col_scan(sjhip_ctx *part, uint32_t n, const QCol &c, unsigned long long *totals) {  // (the column's bytes: totals[2])
    scan_lengths<QCol>(part, n, k_q_col_tile_sums, k_q_col_tile_apply, c, nullptr, nullptr, c.tiles, totals);
}
static void col_gather(sjhip_ctx *part, const QView &q, uint32_t n, const QCol &c, u64 *off, u8 *status, Arr<u8> data) {
    hipLaunchKernelGGL(k_q_col_gather, dim3((n + 255) / 256), dim3(256), 0, part->stream, q, c, off, status, data);
}

// The column of every part lives in the part's d_col: offsets [n + 1] (from 0 in every part), status [n], the bytes.
struct ColOut { u64 *off; u8 *status, *data; };
static size_t col_layout(Carve c, size_t n, size_t bytes, ColOut *o) {
    o->off = c.take<u64>(n + 1);
    o->status = c.take<u8>(n);
    o->data = c.take<u8>(bytes);
    return c.used;
}
struct ColumnBuild {
    using Sizes = ResultState::Column;
    using Work = QCol;
    static constexpr auto product = &ResultState::column;
    static constexpr const char *SYNC_MEASURE = "column sync", *SYNC_GATHER = "column gather sync";
    QPath pth;
    uint32_t cvt;
    size_t *records, *bytes;
    bool names = false;  // sjhip_extract_row_names: the names of the member rows in force, no path
    size_t work(Carve c, const sjhip_ctx *, uint32_t n, QCol *col, unsigned long long **totals) const {
        *totals = c.take<unsigned long long>(32);
        col_work(c, n, col);
        return c.used;
    }
    int measure(sjhip_ctx *ctx, sjhip_ctx *part, const QView &q, uint32_t n, const QCol &c, size_t, unsigned long long *totals) const {
        if (names) hipLaunchKernelGGL(k_q_names_len, dim3((n + 1u + 255) / 256), dim3(256), 0, part->stream, q, c);
        else hipLaunchKernelGGL(k_q_col_len, dim3((n + 1u + 255) / 256), dim3(256), 0, part->stream, q, pth, cvt, c);
        col_scan(part, n, c, totals);
        HIPCHK(hipGetLastError(), "column launch");
        HIPCHK(hipMemcpyAsync(part->h_scratch + 512, totals + 2, 8, hipMemcpyDeviceToHost, part->stream), "D2H column bytes");
        return SJHIP_OK;
    }
    Sizes sizes_of(size_t n, const unsigned long long *h) const { return {n, (size_t)h[0]}; }
    void add(Sizes *t, const Sizes &s) const { t->records += s.records, t->bytes += s.bytes; }
    int gather(sjhip_ctx *ctx, sjhip_ctx *part, const QView &q, uint32_t n, const QCol &c, const Sizes &s) const {
        ColOut o;
        const int rc = reserve_layout(part, part->d_col, [&](Carve cv) { return col_layout(cv, n, s.bytes, &o); });
        if (rc) return rc;
        col_gather(part, q, n, c, o.off, o.status, SJ_ARR(o.data, s.bytes, A_COL));
        HIPCHK(hipGetLastError(), "column gather launch");
        return SJHIP_OK;
    }
    void finish(Sizes *total) const { *records = total->records, *bytes = total->bytes; }
};

int sjhip_extract_path_strings(sjhip_ctx *ctx, const uint8_t *keys, const uint32_t *key_lens, uint32_t n_keys, uint32_t flags,
                               size_t *records, size_t *bytes) {
    if (!records || !bytes || (flags & ~SJHIP_COL_CVT)) return SJHIP_ERR_ARG;
    ColumnBuild p;
    p.cvt = flags & SJHIP_COL_CVT, p.records = records, p.bytes = bytes;
    size_t klen = 0;
    const int rc = make_path(ctx, keys, key_lens, n_keys, &p.pth, &klen);
    return rc ? rc : build_product(ctx, keys, klen, p);
}

int sjhip_fetch_path_strings(sjhip_ctx *ctx, uint64_t *offsets, uint8_t *data, uint8_t *status) {
    if (!ctx) return SJHIP_ERR_ARG;
    if (!ctx->res.column.exists())
        return no_product(ctx, "no string column on the device (sjhip_fetch_path_strings follows sjhip_extract_path_strings, with no parse in between)");
    const Seg segs[] = {{offsets, 8, RECORDS, BYTES, "D2H column offsets"},
                        {status, 1, RECORDS, NO_DOM, "D2H column status"},
                        {data, 1, BYTES, NO_DOM, "D2H column bytes"}};
    // (this fetch ends without query_bounds_check, unlike the list's and the table's: the debug build reports a violation of
    // k_q_col_gather with the next checked query call -- it has been so since the column was added, and stays so)
    return fetch_joined(ctx, "column fetch sync", segs, 3,
        [](sjhip_ctx *part, size_t *count, const void **src) {
            const ResultState::Column &s = part->res.column.sizes();
            ColOut o;
            (void)col_layout(Carve(part->d_col.p), s.records, s.bytes, &o);
            count[RECORDS] = s.records, count[BYTES] = s.bytes;
            src[0] = o.off, src[1] = o.status, src[2] = o.data;
        },
        [&](const size_t *total) { return !offsets || !status || (!data && total[BYTES]) ? SJHIP_ERR_ARG : SJHIP_OK; });
}

// ---- list columns --------------------------------------------------------------------------------------------------------------
// The list column of every part lives in the part's d_list, an arena of its own (d_col keeps the string column): list offsets
// [n + 1] (from 0 in every part), status [n], then the values [elems], or the string offsets [elems + 1] (from 0) and the bytes;
// the work arrays of the three steps (QList) in its d_kat, which only lives for one call.
struct ListOut { u64 *off, *values, *soff; u8 *status, *data; };
static size_t list_layout(Carve c, size_t n, size_t elems, size_t bytes, bool strings, ListOut *o) {
    o->off = c.take<u64>(n + 1);
    o->status = c.take<u8>(n);
    o->values = strings ? nullptr : c.take<u64>(elems);
    o->soff = strings ? c.take<u64>(elems + 1) : nullptr;
    o->data = strings ? c.take<u8>(bytes) : nullptr;
    return c.used;
}
struct ListBuild {
    using Sizes = ResultState::ListColumn;
    using Work = QList;
    static constexpr auto product = &ResultState::list;
    static constexpr const char *SYNC_MEASURE = "list column sync", *SYNC_GATHER = "list gather sync";
    QPath pth;
    int mode;  // SJHIP_COL_FLOAT / INT / UINT, LIST_STR or LIST_CVT
    size_t *records, *elems, *bytes;
    bool strings() const { return mode >= LIST_STR; }
    size_t work(Carve c, const sjhip_ctx *, uint32_t n, QList *l, unsigned long long **totals) const {
        *totals = c.take<unsigned long long>(32);
        l->idx = c.take<u64>(n);
        l->cnt = c.take<u64>((size_t)n + 1);
        l->bytes = strings() ? c.take<u64>((size_t)n + 1) : nullptr;
        l->status = c.take<u8>(n);
        l->tiles_c = c.take<unsigned long long>(tiles_of(n));
        l->tiles_b = strings() ? c.take<unsigned long long>(tiles_of(n)) : nullptr;
        return c.used;
    }
    // the conversion check, the counts (and the bytes of strings) and their scans: the elements in totals[0], the bytes in [1]
    int measure(sjhip_ctx *ctx, sjhip_ctx *part, const QView &q, uint32_t n, const QList &l, size_t, unsigned long long *totals) const {
        const dim3 grid((n + 1u + 255) / 256), block(256);
        HIPCHK(hipMemsetAsync(totals, 0, 16, part->stream), "list totals memset");
        if (mode == LIST_CVT) hipLaunchKernelGGL(k_q_list_measure_cvt, grid, block, 0, part->stream, q, pth, l);
        else hipLaunchKernelGGL(k_q_list_measure, grid, block, 0, part->stream, q, pth, mode, l);
        scan_lengths<QList>(part, n, k_q_list_tile_sums, k_q_list_tile_apply, l, l.tiles_c, l.tiles_b, nullptr, totals);
        HIPCHK(hipGetLastError(), "list column launch");
        HIPCHK(hipMemcpyAsync(part->h_scratch + 512, totals, 16, hipMemcpyDeviceToHost, part->stream), "D2H list totals");
        return SJHIP_OK;
    }
    Sizes sizes_of(size_t n, const unsigned long long *h) const { return {n, (size_t)h[0], strings() ? (size_t)h[1] : 0, strings()}; }
    void add(Sizes *t, const Sizes &s) const { t->records += s.records, t->elems += s.elems, t->bytes += s.bytes; }
    int gather(sjhip_ctx *ctx, sjhip_ctx *part, const QView &q, uint32_t n, const QList &l, const Sizes &s) const {
        ListOut o;
        const size_t ne = s.elems, nb = s.bytes;
        const int rc = reserve_layout(part, part->d_list, [&](Carve cv) { return list_layout(cv, n, ne, nb, strings(), &o); });
        if (rc) return rc;
        const dim3 grid((n + 255) / 256), block(256);
        if (!strings())
            hipLaunchKernelGGL(k_q_list_gather_num, grid, block, 0, part->stream, q, l, mode, o.off, o.status, SJ_ARR(o.values, ne, A_LIST_VAL));
        else if (mode == LIST_STR)
            hipLaunchKernelGGL(k_q_list_gather_str, grid, block, 0, part->stream, q, l, o.off, o.status,
                               SJ_ARR(o.soff, ne + 1, A_LIST_SOFF), SJ_ARR(o.data, nb, A_LIST_DATA));
        else
            hipLaunchKernelGGL(k_q_list_gather_cvt, grid, block, 0, part->stream, q, l, o.off, o.status,
                               SJ_ARR(o.soff, ne + 1, A_LIST_SOFF), SJ_ARR(o.data, nb, A_LIST_DATA));
        HIPCHK(hipGetLastError(), "list gather launch");
        return SJHIP_OK;
    }
    void finish(Sizes *total) const {
        total->strings = strings();
        *records = total->records, *elems = total->elems;
        if (bytes) *bytes = total->bytes;
    }
};
static int list_extract(sjhip_ctx *ctx, const uint8_t *keys, const uint32_t *key_lens, uint32_t n_keys, int mode, size_t *records,
                        size_t *elems, size_t *bytes) {
    ListBuild p;
    p.mode = mode, p.records = records, p.elems = elems, p.bytes = bytes;
    size_t klen = 0;
    const int rc = make_path(ctx, keys, key_lens, n_keys, &p.pth, &klen);
    return rc ? rc : build_product(ctx, keys, klen, p);
}

int sjhip_extract_path_list(sjhip_ctx *ctx, const uint8_t *keys, const uint32_t *key_lens, uint32_t n_keys, int kind, size_t *records,
                            size_t *elems) {
    if (!records || !elems) return SJHIP_ERR_ARG;
    if (kind < SJHIP_COL_FLOAT || kind > SJHIP_COL_UINT) {
        if (ctx) ctx_set_error(ctx, "sjhip_extract_path_list: kind %d (the reference's arrays convert to float, integer and unsigned integer)", kind);
        return SJHIP_ERR_ARG;
    }
    return list_extract(ctx, keys, key_lens, n_keys, kind, records, elems, nullptr);
}
int sjhip_extract_path_list_strings(sjhip_ctx *ctx, const uint8_t *keys, const uint32_t *key_lens, uint32_t n_keys, uint32_t flags,
                                    size_t *records, size_t *elems, size_t *bytes) {
    if (!records || !elems || !bytes || (flags & ~SJHIP_COL_CVT)) return SJHIP_ERR_ARG;
    return list_extract(ctx, keys, key_lens, n_keys, (flags & SJHIP_COL_CVT) ? LIST_CVT : LIST_STR, records, elems, bytes);
}

// inner: the values (numbers) or the string offsets (strings) of the elements.  Two offset arrays over two domains: the list
// offsets are indexed by records and count elements, the string offsets are indexed by elements and count bytes.
static int list_fetch(sjhip_ctx *ctx, bool strings, uint64_t *list_offsets, uint64_t *inner, uint8_t *data, uint8_t *status) {
    if (!ctx) return SJHIP_ERR_ARG;
    if (!ctx->res.list_of(strings))  // (... or it is of the other kind)
        return no_product(ctx, "no list column of this kind on the device (sjhip_fetch_path_list follows sjhip_extract_path_list, "
                               "sjhip_fetch_path_list_strings follows sjhip_extract_path_list_strings, with no parse in between)");
    const Seg segs[] = {{list_offsets, 8, RECORDS, ELEMS, "D2H list offsets"},
                        {status, 1, RECORDS, NO_DOM, "D2H list status"},
                        {inner, 8, ELEMS, strings ? BYTES : NO_DOM, "D2H list elements"},
                        {data, 1, BYTES, NO_DOM, "D2H list bytes"}};
    const int rc = fetch_joined(ctx, "list fetch sync", segs, 4,
        [&](sjhip_ctx *part, size_t *count, const void **src) {
            const ResultState::ListColumn &s = part->res.list.sizes();
            ListOut o;
            (void)list_layout(Carve(part->d_list.p), s.records, s.elems, s.bytes, strings, &o);
            count[RECORDS] = s.records, count[ELEMS] = s.elems, count[BYTES] = s.bytes;
            src[0] = o.off, src[1] = o.status, src[2] = strings ? o.soff : o.values, src[3] = o.data;
        },
        [&](const size_t *total) {
            const bool null = !list_offsets || !status || (!inner && (strings || total[ELEMS])) || (strings && !data && total[BYTES]);
            return null ? SJHIP_ERR_ARG : SJHIP_OK;
        });
    return rc ? rc : query_bounds_check(ctx);  // (debug build: the gather kernel has finished here)
}
int sjhip_fetch_path_list(sjhip_ctx *ctx, uint64_t *list_offsets, void *values, uint8_t *status) {
    return list_fetch(ctx, false, list_offsets, (uint64_t *)values, nullptr, status);
}
int sjhip_fetch_path_list_strings(sjhip_ctx *ctx, uint64_t *list_offsets, uint64_t *str_offsets, uint8_t *data, uint8_t *status) {
    return list_fetch(ctx, true, list_offsets, str_offsets, data, status);
}

// ---- tables ---------------------------------------------------------------------------------------------------------------------
// The table of every part lives in arenas of its own.  d_table, laid out from the record count and the kinds before the walk that
// fills it: values [n] and status [n] of every numeric / bool column, offsets [n + 1] (from 0 in every part) and status [n] of
// every string column.  d_tabledata, laid out once the walk and the scans have said how long the texts are: the bytes of the
// string columns, one after another.  The work arrays of the string columns (a QCol each) are in d_kat, which lives for one call.
struct TableOut {
    u8 *val[TABLE_MAX_COLS];   // numeric / bool
    u64 *off[TABLE_MAX_COLS];  // strings
    u8 *status[TABLE_MAX_COLS];
    u8 *data[TABLE_MAX_COLS];  // strings: in d_tabledata
};
static bool table_is_string(int kind) { return kind > SJHIP_COL_BOOL; }
static size_t table_layout(Carve c, size_t n, uint32_t n_cols, const uint8_t *kind, TableOut *o) {
    for (uint32_t j = 0; j < n_cols; j++) {
        o->val[j] = nullptr;
        o->off[j] = nullptr;
        if (table_is_string(kind[j])) o->off[j] = c.take<u64>(n + 1);
        else o->val[j] = c.take<u8>(n * (kind[j] == SJHIP_COL_BOOL ? 1u : 8u));
        o->status[j] = c.take<u8>(n);
    }
    return c.used;
}
static size_t table_data_layout(Carve c, uint32_t n_cols, const uint8_t *kind, const size_t *bytes, TableOut *o) {
    for (uint32_t j = 0; j < n_cols; j++) o->data[j] = table_is_string(kind[j]) ? c.take<u8>(bytes[j]) : nullptr;
    return c.used;
}
struct TableBuild {
    using Sizes = ResultState::Table;
    struct Work { QCol c[TABLE_MAX_COLS]; };  // (of the string columns)
    static constexpr auto product = &ResultState::table;
    static constexpr const char *SYNC_MEASURE = "table sync", *SYNC_GATHER = "table gather sync";
    QTable t;
    uint32_t n_cols;
    size_t *records, *bytes;
    bool is_string(uint32_t j) const { return table_is_string(t.pl.kind[j]); }
    size_t work(Carve c, const sjhip_ctx *, uint32_t n, Work *w, unsigned long long **totals) const {
        *totals = c.take<unsigned long long>(4 * TABLE_MAX_COLS);  // (col_scan leaves column j's bytes in entry 4 j + 2)
        for (uint32_t j = 0; j < n_cols; j++)
            if (is_string(j)) col_work(c, n, &w->c[j]);
        return c.used;
    }
    // d_table for the record count; the walk, which fills it and the string columns' lengths; their scans
    int measure(sjhip_ctx *ctx, sjhip_ctx *part, const QView &q, uint32_t n, const Work &w, size_t work_bytes, unsigned long long *totals) const {
        TableOut o;
        size_t out_bytes = 0;
        const int rc = reserve_layout(part, part->d_table, [&](Carve cv) { return table_layout(cv, n, n_cols, t.pl.kind, &o); }, &out_bytes);
        if (rc) return rc;
        u8 *const out = (u8 *)part->d_table.p, *const kat = (u8 *)part->d_kat.p;
        QTable tk = t;
        tk.out = SJ_ARR(out, out_bytes, A_TABLE_OUT);
        tk.work = SJ_ARR(kat, work_bytes, A_TABLE_WORK);
        for (uint32_t j = 0; j < n_cols; j++) {
            const bool str = is_string(j);
            tk.a_off[j] = str ? (u64)((u8 *)w.c[j].idx - kat) : (u64)(o.val[j] - out);
            tk.b_off[j] = str ? (u64)((u8 *)w.c[j].off - kat) : 0;
            tk.st_off[j] = str ? (u64)(w.c[j].status - kat) : (u64)(o.status[j] - out);
        }
        hipLaunchKernelGGL(k_q_table_walk, dim3((n + 1u + 255) / 256), dim3(256), 0, part->stream, q, tk);
        for (uint32_t j = 0; j < n_cols; j++)
            if (is_string(j)) col_scan(part, n, w.c[j], totals + 4 * j);
        HIPCHK(hipGetLastError(), "table launch");
        HIPCHK(hipMemcpyAsync(part->h_scratch + 512, totals, 4 * TABLE_MAX_COLS * 8, hipMemcpyDeviceToHost, part->stream), "D2H table bytes");
        return SJHIP_OK;
    }
    Sizes sizes_of(size_t n, const unsigned long long *h) const {
        Sizes s;
        s.records = n, s.n_cols = n_cols;
        for (uint32_t j = 0; j < n_cols; j++) {
            s.kind[j] = t.pl.kind[j];
            s.bytes[j] = is_string(j) ? (size_t)h[4 * j + 2] : 0;
        }
        return s;
    }
    void add(Sizes *tot, const Sizes &s) const {
        tot->records += s.records;
        for (uint32_t j = 0; j < n_cols; j++) tot->bytes[j] += s.bytes[j];
    }
    // the gathers of the string columns, into the part's d_tabledata
    int gather(sjhip_ctx *ctx, sjhip_ctx *part, const QView &q, uint32_t n, const Work &w, const Sizes &s) const {
        TableOut o;
        const int rc = reserve_layout(part, part->d_tabledata, [&](Carve cv) { return table_data_layout(cv, n_cols, s.kind, s.bytes, &o); });
        if (rc) return rc;
        (void)table_layout(Carve(part->d_table.p), n, n_cols, s.kind, &o);
        for (uint32_t j = 0; j < n_cols; j++) {
            if (!is_string(j)) continue;
            u8 *const data = o.data[j];
            col_gather(part, q, n, w.c[j], o.off[j], o.status[j], SJ_ARR(data, s.bytes[j], A_TABLE_DATA));
        }
        HIPCHK(hipGetLastError(), "table gather launch");
        return SJHIP_OK;
    }
    void finish(Sizes *total) const {
        total->n_cols = n_cols, *records = total->records;
        memcpy(total->kind, t.pl.kind, n_cols);
        for (uint32_t j = 0; j < n_cols; j++) bytes[j] = total->bytes[j];
    }
};

int sjhip_extract_table(sjhip_ctx *ctx, const uint8_t *keys, const uint32_t *key_lens, const uint32_t *path_lens, const int *kinds,
                        uint32_t n_cols, size_t *records, size_t *bytes) {
    if (!ctx) return SJHIP_ERR_ARG;
    if (!keys || !key_lens || !path_lens || !kinds || !records || !bytes) {
        ctx_set_error(ctx, "sjhip_extract_table: a null argument");
        return SJHIP_ERR_ARG;
    }
    TableBuild p;
    p.n_cols = n_cols, p.records = records, p.bytes = bytes;
    uint8_t blob[TABLE_MAX_BYTES];
    uint32_t blob_len = 0, bad_col = 0;
    const int why = table_plan(keys, key_lens, path_lens, kinds, n_cols, &p.t.pl, blob, &blob_len, &bad_col);
    if (why) {
        ctx_set_error(ctx, "sjhip_extract_table: %s (%u columns, found at column %u)", table_plan_error(why), n_cols, bad_col);
        return SJHIP_ERR_ARG;
    }
    return build_product(ctx, blob, blob_len, p);
}

int sjhip_fetch_table_column(sjhip_ctx *ctx, uint32_t col, void *values, uint64_t *offsets, uint8_t *data, uint8_t *status) {
    if (!ctx) return SJHIP_ERR_ARG;
    if (!ctx->res.table.exists())
        return no_product(ctx, "no table on the device (sjhip_fetch_table_column follows sjhip_extract_table, with no parse in between)");
    const ResultState::Table &all = ctx->res.table.sizes();
    if (col >= all.n_cols) {
        ctx_set_error(ctx, "sjhip_fetch_table_column: column %u of a table of %u columns", col, all.n_cols);
        return SJHIP_ERR_ARG;
    }
    const int kind = all.kind[col];
    const bool str = table_is_string(kind);
    const Seg status_seg = {status, 1, RECORDS, NO_DOM, "D2H table status"};
    const Seg num_segs[] = {status_seg, {values, kind == SJHIP_COL_BOOL ? 1u : 8u, RECORDS, NO_DOM, "D2H table values"}};
    const Seg str_segs[] = {status_seg, {offsets, 8, RECORDS, BYTES, "D2H table offsets"}, {data, 1, BYTES, NO_DOM, "D2H table bytes"}};
    const int rc = fetch_joined(ctx, "table fetch sync", str ? str_segs : num_segs, str ? 3 : 2,
        [&](sjhip_ctx *part, size_t *count, const void **src) {
            const ResultState::Table &s = part->res.table.sizes();
            TableOut o;
            (void)table_layout(Carve(part->d_table.p), s.records, s.n_cols, s.kind, &o);
            (void)table_data_layout(Carve(part->d_tabledata.p), s.n_cols, s.kind, s.bytes, &o);
            count[RECORDS] = s.records, count[BYTES] = s.bytes[col];
            src[0] = o.status[col], src[1] = str ? (const void *)o.off[col] : o.val[col], src[2] = o.data[col];
        },
        [&](const size_t *total) {
            if (status && (str ? offsets && (data || !total[BYTES]) : values != nullptr)) return SJHIP_OK;
            ctx_set_error(ctx, "sjhip_fetch_table_column: a null destination for column %u (%s)", col, str ? "offsets, data, status" : "values, status");
            return SJHIP_ERR_ARG;
        });
    return rc ? rc : query_bounds_check(ctx);  // (debug build: the kernels of sjhip_extract_table have finished here)
}

// ---- row selection ---------------------------------------------------------------------------------------------------------------
// The selection of every part lives in the part's d_rows, an arena of its own (rows_layout): row offsets [n + 1] over the part's n
// records (from 0 in every part), status [n], the row index [rows] in merged tape indices.  It is built over the RECORDS -- the
// selection it replaces is given up first (build_product) -- with the work arrays of its passes (QRows) in d_kat; the measure
// counts the rows, the gather writes them.  While the owner's product exists, make_view hands the row index to the path queries.
struct RowsBuild {
    using Sizes = ResultState::Rows;
    using Work = QRows;
    static constexpr auto product = &ResultState::rows;
    static constexpr const char *SYNC_MEASURE = "row selection sync", *SYNC_GATHER = "row gather sync";
    QPath pth;
    size_t *records, *rows;
    static u32 tape_tiles(const sjhip_ctx *part) { return (u32)((part->tape_len + TW_TILE - 1) / TW_TILE); }
    size_t work(Carve c, const sjhip_ctx *part, uint32_t n, QRows *w, unsigned long long **totals) const {
        const u32 tiles = tape_tiles(part);
        *totals = w->totals = c.take<unsigned long long>(32);
        w->open = c.take<u64>(n);
        w->close = c.take<u64>(n);
        w->status = c.take<u8>(n);
        w->depth = c.take<unsigned long long>(tiles);
        w->cnt = c.take<unsigned long long>(tiles);
        w->tile_last = c.take<long long>(tiles);
        w->depth_want = pth.n + 1u;
        return c.used;
    }
    int measure(sjhip_ctx *ctx, sjhip_ctx *part, const QView &q, uint32_t n, const QRows &w, size_t, unsigned long long *totals) const {
        const dim3 tiles(tape_tiles(part)), block(TW_THREADS), one(1), wide(1024);
        unsigned long long *const none = nullptr;
        const Arr<u64> no_index = SJ_ARR((u64 *)nullptr, 0, A_ROWS);
        HIPCHK(hipMemsetAsync(totals, 0, 256, part->stream), "row totals memset");
        hipLaunchKernelGGL(k_q_rows_records, dim3((n + 255) / 256), dim3(256), 0, part->stream, q, pth, w);
        hipLaunchKernelGGL(k_q_rows_tile<0>, tiles, block, 0, part->stream, q, w, 0u, no_index);
        hipLaunchKernelGGL(k_q_rows_last, tiles, block, 0, part->stream, q, w);  // (these three end at once unless a tile asked)
        hipLaunchKernelGGL(k_q_rows_scan_last, one, wide, 0, part->stream, w, tiles.x);
        hipLaunchKernelGGL(k_q_rows_tile<0>, tiles, block, 0, part->stream, q, w, 1u, no_index);
        hipLaunchKernelGGL(k_tw_scan_sums, one, wide, 0, part->stream, w.depth, none, none, tiles.x, totals);
        hipLaunchKernelGGL(k_q_rows_tile<1>, tiles, block, 0, part->stream, q, w, 0u, no_index);
        hipLaunchKernelGGL(k_tw_scan_sums, one, wide, 0, part->stream, none, w.cnt, none, tiles.x, totals);  // the rows: totals[1]
        HIPCHK(hipGetLastError(), "row selection launch");
        HIPCHK(hipMemcpyAsync(part->h_scratch + 512, totals + 1, 8, hipMemcpyDeviceToHost, part->stream), "D2H row count");
        return SJHIP_OK;
    }
    Sizes sizes_of(size_t n, const unsigned long long *h) const { return {n, (size_t)h[0], pth.n + 1u}; }
    void add(Sizes *t, const Sizes &s) const { t->records += s.records, t->rows += s.rows, t->depth = s.depth; }
    int gather(sjhip_ctx *ctx, sjhip_ctx *part, const QView &q, uint32_t n, const QRows &w, const Sizes &s) const {
        RowsOut o;
        const int rc = reserve_layout(part, part->d_rows, [&](Carve cv) { return rows_layout(cv, n, s.rows, &o); });
        if (rc) return rc;
        if (s.rows)
            hipLaunchKernelGGL(k_q_rows_tile<2>, dim3(tape_tiles(part)), dim3(TW_THREADS), 0, part->stream, q, w, 0u, SJ_ARR(o.index, s.rows, A_ROWS));
        hipLaunchKernelGGL(k_q_rows_offsets, dim3((n + 255) / 256), dim3(256), 0, part->stream, q, w, SJ_ARR((const u64 *)o.index, s.rows, A_ROWS),
                           (u64)s.rows, o.off, o.status);
        HIPCHK(hipGetLastError(), "row gather launch");
        return SJHIP_OK;
    }
    void finish(Sizes *total) const { *records = total->records, *rows = total->rows; }
};

int sjhip_select_rows(sjhip_ctx *ctx, const uint8_t *keys, const uint32_t *key_lens, uint32_t n_keys, size_t *records, size_t *rows) {
    if (!records || !rows) return SJHIP_ERR_ARG;
    RowsBuild p;
    p.records = records, p.rows = rows;
    size_t klen = 0;
    const int rc = make_path(ctx, keys, key_lens, n_keys, &p.pth, &klen, true);
    return rc ? rc : build_product(ctx, keys ? keys : &NO_VALUE, klen, p);
}

int sjhip_fetch_rows(sjhip_ctx *ctx, uint64_t *row_offsets, uint64_t *row_index, uint8_t *status) {
    if (!ctx) return SJHIP_ERR_ARG;
    if (!ctx->res.rows.exists())
        return no_product(ctx, "no row selection on the device (sjhip_fetch_rows follows sjhip_select_rows, with no parse and no sjhip_select_records in between)");
    const Seg segs[] = {{row_offsets, 8, RECORDS, ELEMS, "D2H row offsets"},
                        {status, 1, RECORDS, NO_DOM, "D2H row status"},
                        {row_index, 8, ELEMS, NO_DOM, "D2H row index"}};
    const int rc = fetch_joined(ctx, "row fetch sync", segs, 3,
        [](sjhip_ctx *part, size_t *count, const void **src) {
            const ResultState::Rows &s = part->res.rows.sizes();
            RowsOut o;
            (void)rows_layout(Carve(part->d_rows.p), s.records, s.rows, &o);
            count[RECORDS] = s.records, count[ELEMS] = s.rows;
            src[0] = o.off, src[1] = o.status, src[2] = o.index;
        },
        [](const size_t *) { return SJHIP_OK; });  // (any destination may be null: that array is not copied)
    return rc ? rc : query_bounds_check(ctx);  // (debug build: the kernels of sjhip_select_rows have finished here)
}

int sjhip_select_records(sjhip_ctx *ctx) {
    if (!ctx) return SJHIP_ERR_ARG;
    ctx->res.rows.begin();
    for (sjhip_ctx *part : result_parts(ctx)) part->res.rows.begin();
    return SJHIP_OK;
}

// ---- row predicates ----------------------------------------------------------------------------------------------------------------
// sjhip_where_path narrows the selection of every part in place: the old selection -- or, without one, the records -- is what the
// passes run on (make_view, on_rows) until the new one is published over it.  Two passes over the parts, the shape of
// build_product, but nothing is given up first: pass 1 marks and counts (the kept rows of the part come back through
// h_scratch + 512), pass 2 compacts into the work arena -- laid out in pass 1 for every row kept -- and copies offsets, statuses
// and index into d_rows behind the kernels, which is reserved here only when there was no selection (a narrowed one fits where
// the old one lies, and rows_layout keeps offsets and statuses in their place).
struct WhereNew { u64 *index, *off; u8 *status; };  // the new selection of a part, in its d_kat
// The work arrays of a narrowing over the n rows of a part, in the part's d_kat: the totals of the scan in front, the tile sums, the
// flags and their prefix, and the new selection.  (sjhip_order_path lays them out behind its own.)
static size_t where_layout(Carve c, const sjhip_ctx *part, uint32_t n, QWhere *w, WhereNew *nw, unsigned long long **totals) {
    const size_t recs = (size_t)part->q_records + 1u;
    *totals = c.take<unsigned long long>(32);
    w->tiles = c.take<unsigned long long>((n + QTILE - 1) / QTILE);
    u8 *const flag = c.take<u8>(n);
    u32 *const pre = c.take<u32>(n);
    w->flag = SJ_ARR(flag, n, A_WHERE_FLAG);
    w->pre = SJ_ARR(pre, n, A_WHERE_PRE);
    nw->index = c.take<u64>(n);  // (room for every row: the count is not known yet)
    nw->off = c.take<u64>(recs + 1);
    nw->status = c.take<u8>(recs);
    return c.used;
}
// The second half of a narrowing, whoever marked: work[k].flag holds the keep flag of every row of part k, work[k].tiles the
// exclusive prefix of the kept rows per tile and kept[k] their number (all of a part without rows: untouched, 0).  The rows are
// compacted into fresh[k], copied over the selection in d_rows, and the new selection is published.  (Nothing of d_kat is asked
// for: the arrays stay where the caller laid them out.)
static int where_narrow(sjhip_ctx *ctx, const std::vector<sjhip_ctx *> &parts, const uint8_t *keys, size_t klen, const uint8_t *val,
                        size_t vlen, const std::vector<QWhere> &work, const std::vector<WhereNew> &fresh, const std::vector<size_t> &kept,
                        size_t *records, size_t *rows) {
    const bool sel = selected(ctx, true);
    int rc = query_over_parts(ctx, parts, keys, klen, val, vlen, true, "row predicate gather sync", [](const sjhip_ctx *, uint32_t) { return (size_t)0; },
        [&](size_t k, sjhip_ctx *part, const QView &q, uint32_t n) -> int {
            const size_t recs = (size_t)part->q_records + 1u;
            RowsOut old, o;
            QWhere w = work[k];
            w.index = SJ_ARR(fresh[k].index, kept[k], A_ROWS);
            w.off = SJ_ARR(fresh[k].off, recs + 1, A_WHERE_OFF);
            w.status = fresh[k].status;
            w.old_off = nullptr;
            w.old_status = nullptr;
            if (sel) {
                const ResultState::Rows &z = part->res.rows.sizes();
                (void)rows_layout(Carve(part->d_rows.p), z.records, z.rows, &old);
                w.old_off = SJ_ARR((const u64 *)old.off, z.records + 1, A_WHERE_OFF);
                w.old_status = old.status;
                (void)rows_layout(Carve(part->d_rows.p), recs, kept[k], &o);
            } else {
                const int rc = reserve_layout(part, part->d_rows, [&](Carve cv) { return rows_layout(cv, recs, kept[k], &o); });
                if (rc) return rc;
            }
            hipLaunchKernelGGL(k_q_where_apply, dim3((n + QTILE - 1) / QTILE), dim3(QT), 0, part->stream, q, w);
            hipLaunchKernelGGL(k_q_where_offsets, dim3(((u32)recs + 255) / 256), dim3(256), 0, part->stream, q, w, (u64)kept[k]);
            HIPCHK(hipGetLastError(), "row predicate gather launch");
            HIPCHK(hipMemcpyAsync(o.off, fresh[k].off, (recs + 1) * 8, hipMemcpyDeviceToDevice, part->stream), "row offsets copy");
            HIPCHK(hipMemcpyAsync(o.status, fresh[k].status, recs, hipMemcpyDeviceToDevice, part->stream), "row status copy");
            if (kept[k])
                HIPCHK(hipMemcpyAsync(o.index, fresh[k].index, kept[k] * 8, hipMemcpyDeviceToDevice, part->stream), "row index copy");
            return SJHIP_OK;
        },
        [](size_t, sjhip_ctx *) {});
    if (rc) return rc;
    ResultState::Rows total;
    total.depth = sel ? ctx->res.rows.sizes().depth : 0u;  // (the rows keep their depth; the root values of the records lie at 0)
    total.members = sel && ctx->res.rows.sizes().members;   // (... and their names: nothing is stored per row)
    bool ok = true;  // (a part without rows launched nothing and is republished as it was: its records, no rows)
    for (size_t k = 0; k < parts.size(); k++) {
        const ResultState::Rows s = {(size_t)parts[k]->q_records + 1u, kept[k], total.depth, total.members};
        ok &= parts[k]->res.publish(&ResultState::rows, s);
        total.records += s.records, total.rows += s.rows;
    }
    if (ctx->res.sharded()) ok &= ctx->res.publish(&ResultState::rows, total);
    *records = total.records, *rows = total.rows;
    return published(ctx, ok);
}
// The first half of sjhip_where_path and sjhip_where_paths: mark(part, q, n, work) launches the kernel that flags the n rows of
// the part and counts the kept ones per tile; they are added up; then the narrowing above.
template <typename M>
static int where_build(sjhip_ctx *ctx, const std::vector<sjhip_ctx *> &parts, const uint8_t *keys, size_t klen, const uint8_t *val,
                       size_t vlen, M mark, size_t *records, size_t *rows) {
    std::vector<QWhere> work(parts.size());
    std::vector<WhereNew> fresh(parts.size());
    std::vector<size_t> kept(parts.size(), 0);
    const int rc = query_over_parts(ctx, parts, keys, klen, val, vlen, true, "row predicate sync",
        [&](const sjhip_ctx *part, uint32_t n) {
            QWhere w;
            WhereNew nw;
            unsigned long long *totals;
            return where_layout(Carve(), part, n, &w, &nw, &totals) + 64;
        },
        [&](size_t k, sjhip_ctx *part, const QView &q, uint32_t n) -> int {
            unsigned long long *totals, *const none = nullptr;
            (void)where_layout(Carve(part->d_kat.p), part, n, &work[k], &fresh[k], &totals);
            const u32 tiles = (n + QTILE - 1) / QTILE;
            HIPCHK(hipMemsetAsync(totals, 0, 256, part->stream), "row predicate totals memset");
            HIPCHK(hipMemsetAsync(work[k].tiles, 0, (size_t)tiles * 8, part->stream), "row predicate tiles memset");
            mark(part, q, n, work[k]);
            hipLaunchKernelGGL(k_tw_scan_sums, dim3(1), dim3(1024), 0, part->stream, work[k].tiles, none, none, tiles, totals);
            HIPCHK(hipGetLastError(), "row predicate launch");
            HIPCHK(hipMemcpyAsync(part->h_scratch + 512, totals, 8, hipMemcpyDeviceToHost, part->stream), "D2H kept rows");
            return SJHIP_OK;
        },
        [&](size_t k, sjhip_ctx *part) {
            kept[k] = part_rows(ctx, part, true) ? (size_t)*(const unsigned long long *)(part->h_scratch + 512) : 0;
        });
    return rc ? rc : where_narrow(ctx, parts, keys, klen, val, vlen, work, fresh, kept, records, rows);
}

// a narrowing that failed half-built: the old selection may have been written over, so it is given up
static int where_gave_up(sjhip_ctx *ctx, const std::vector<sjhip_ctx *> &parts, const char *who, int rc) {
    ctx->res.rows.begin();
    for (sjhip_ctx *part : parts) part->res.rows.begin();
    char why[sizeof ctx->err];
    snprintf(why, sizeof why, "%s", ctx->err);
    ctx_set_error(ctx, "%s failed and the row selection was given up: %.180s", who, why);
    return rc;
}

int sjhip_where_path(sjhip_ctx *ctx, const uint8_t *keys, const uint32_t *key_lens, uint32_t n_keys, int op, const void *value,
                     size_t vlen, uint32_t flags, size_t *records, size_t *rows) {
    if (!ctx || !records || !rows) return SJHIP_ERR_ARG;
    if (flags & ~SJHIP_WHERE_NOT) {
        ctx_set_error(ctx, "sjhip_where_path: unknown flag bits 0x%x", flags & ~SJHIP_WHERE_NOT);
        return SJHIP_ERR_ARG;
    }
    bool is_str = false;
    u64 want = 0;
    int rc = predicate_value(op, value, vlen, &want, &is_str);
    if (rc) {
        ctx_set_error(ctx, "sjhip_where_path: operator %d with a value of %zu bytes", op, vlen);
        return rc;
    }
    QPath pth;
    size_t klen = 0;
    rc = make_path(ctx, keys, key_lens, n_keys, &pth, &klen, true);
    if (rc) return rc;
    const uint8_t *const kb = keys ? keys : &NO_VALUE, *const vb = is_str && value ? (const uint8_t *)value : &NO_VALUE;
    const size_t vl = is_str ? vlen : 0;
    std::vector<sjhip_ctx *> parts;
    rc = query_parts(ctx, kb, klen, vb, vl, &parts);
    if (rc) return rc;  // (nothing has been queued: the selection is as it was)
    const u32 negate = flags & SJHIP_WHERE_NOT;
    rc = where_build(ctx, parts, kb, klen, vb, vl,
                     [&](sjhip_ctx *part, const QView &q, uint32_t n, const QWhere &w) {
                         hipLaunchKernelGGL(k_q_where_mark, dim3((n + 255) / 256), dim3(256), 0, part->stream, q, pth, op, want, negate, w);
                     },
                     records, rows);
    return rc ? where_gave_up(ctx, parts, "sjhip_where_path", rc) : rc;
}

// ---- row predicates of several tests (sjhip_where_paths, sjhip_count_where_paths) -------------------------------------------------
// The arguments of both calls, checked in the order the header names them, become the plan (sj_where.h), the keys of its trie
// and the values end to end -- what travels in QView::key and QView::val.  Nothing of the context is touched here.
struct WhereMulti {
    WherePlan plan;
    uint8_t keys[TABLE_MAX_BYTES];
    uint32_t klen;
    const uint8_t *vals;
    size_t vlen;
};
static int where_multi_plan(sjhip_ctx *ctx, const char *who, const uint8_t *keys, const uint32_t *key_lens, const uint32_t *path_lens,
                            const int *ops, const void *values, const uint32_t *value_lens, uint32_t n_preds, const uint8_t *program,
                            uint32_t program_len, WhereMulti *m) {
    if (n_preds < 1 || n_preds > (uint32_t)SJHIP_WHERE_MAX_PREDS) {
        ctx_set_error(ctx, "%s: %u predicates (1 to %d)", who, n_preds, SJHIP_WHERE_MAX_PREDS);
        return SJHIP_ERR_ARG;
    }
    if (!path_lens || !ops || !value_lens || !program) {
        ctx_set_error(ctx, "%s: a null argument (path_lens, ops, value_lens, program)", who);
        return SJHIP_ERR_ARG;
    }
    WherePlan &pl = m->plan;
    memset(&pl, 0, sizeof pl);
    // the values: what sjhip_where_path takes for the operator, end to end
    size_t val_at = 0;
    for (uint32_t p = 0; p < n_preds; p++) {
        const uint32_t vl = value_lens[p];
        if (val_at + vl > (size_t)WHERE_MAX_VALUE_BYTES) {
            ctx_set_error(ctx, "%s: predicate %u: the values are longer than %d bytes together", who, p, WHERE_MAX_VALUE_BYTES);
            return SJHIP_ERR_ARG;
        }
        const int op = ops[p];
        if (op < SJHIP_OP_EXISTS || op > SJHIP_OP_PREFIX_STRING) {
            ctx_set_error(ctx, "%s: predicate %u: unknown operator %d", who, p, op);
            return SJHIP_ERR_ARG;
        }
        if (vl && !values) {
            ctx_set_error(ctx, "%s: predicate %u: a value of %u bytes is announced and `values` is null", who, p, vl);
            return SJHIP_ERR_ARG;
        }
        bool is_str = false;
        u64 want = 0;
        const void *const v = vl ? (const void *)((const uint8_t *)values + val_at) : (const void *)&NO_VALUE;
        if (predicate_value(op, v, vl, &want, &is_str) || ((op == SJHIP_OP_EXISTS || op == SJHIP_OP_IS_NULL) && vl)) {
            ctx_set_error(ctx, "%s: predicate %u: operator %d with a value of %u bytes", who, p, op, vl);
            return SJHIP_ERR_ARG;
        }
        pl.op[p] = (uint8_t)op;
        pl.want[p] = want;
        pl.val_b[p] = (uint16_t)val_at;
        pl.val_n[p] = (uint16_t)(is_str ? vl : 0u);
        val_at += vl;
    }
    m->vals = val_at ? (const uint8_t *)values : &NO_VALUE;
    m->vlen = val_at;
    // the paths: the predicates that have one are the columns of a table plan, in their order
    uint32_t col_path_lens[TABLE_MAX_COLS], n_cols = 0;
    int kinds[TABLE_MAX_COLS];
    size_t n_keys = 0;
    for (uint32_t p = 0; p < n_preds; p++) {
        if (path_lens[p] == 0) {
            pl.empty |= (uint16_t)(1u << p);
            continue;
        }
        pl.pred_of_col[n_cols] = (uint8_t)p;
        col_path_lens[n_cols] = path_lens[p];
        kinds[n_cols++] = SJHIP_COL_FLOAT;  // (the walk does not look at the kind of a column)
        n_keys += path_lens[p];
    }
    m->klen = 0;
    if (n_cols) {
        if (!keys || !key_lens) {
            ctx_set_error(ctx, "%s: a null argument (%zu keys are announced)", who, n_keys);
            return SJHIP_ERR_ARG;
        }
        // (the keys of the paths lie end to end whether or not empty paths stand between them: table_plan reads them as they are)
        uint32_t bad_col = 0;
        const int why = table_plan(keys, key_lens, col_path_lens, kinds, n_cols, &pl.pl, m->keys, &m->klen, &bad_col);
        if (why) {
            ctx_set_error(ctx, "%s: predicate %u: %s", who, (unsigned)pl.pred_of_col[bad_col], table_plan_error(why));
            return SJHIP_ERR_ARG;
        }
    }
    uint32_t pos = 0;
    const int why = where_program_check(program, program_len, n_preds, &pos);
    if (why) {
        if (why == WHERE_PROG_UNUSED) ctx_set_error(ctx, "%s: predicate %u: %s", who, pos, where_program_error(why));
        else ctx_set_error(ctx, "%s: program position %u (of %u bytes): %s", who, pos, program_len, where_program_error(why));
        return SJHIP_ERR_ARG;
    }
    pl.n_preds = (uint8_t)n_preds;
    pl.program_len = (uint8_t)program_len;
    memcpy(pl.program, program, program_len);
    return SJHIP_OK;
}
static void where_multi_launch(sjhip_ctx *part, const QView &q, uint32_t n, const WherePlan &plan, const QWhere &w, unsigned long long *count) {
    hipLaunchKernelGGL(k_q_where_multi_mark, dim3((n + 255) / 256), dim3(256), 0, part->stream, q, plan, w, count);
}

int sjhip_where_paths(sjhip_ctx *ctx, const uint8_t *keys, const uint32_t *key_lens, const uint32_t *path_lens, const int *ops,
                      const void *values, const uint32_t *value_lens, uint32_t n_preds, const uint8_t *program, uint32_t program_len,
                      size_t *records, size_t *rows) {
    if (!ctx) return SJHIP_ERR_ARG;
    if (!records || !rows) {
        ctx_set_error(ctx, "sjhip_where_paths: a null size pointer");
        return SJHIP_ERR_ARG;
    }
    WhereMulti m;
    int rc = where_multi_plan(ctx, "sjhip_where_paths", keys, key_lens, path_lens, ops, values, value_lens, n_preds, program, program_len, &m);
    if (rc) return rc;
    std::vector<sjhip_ctx *> parts;
    rc = query_parts(ctx, m.keys, m.klen, m.vals, m.vlen, &parts);
    if (rc) return rc;  // (nothing has been queued: the selection is as it was)
    rc = where_build(ctx, parts, m.keys, m.klen, m.vals, m.vlen,
                     [&](sjhip_ctx *part, const QView &q, uint32_t n, const QWhere &w) { where_multi_launch(part, q, n, m.plan, w, nullptr); },
                     records, rows);
    return rc ? where_gave_up(ctx, parts, "sjhip_where_paths", rc) : rc;
}

int sjhip_count_where_paths(sjhip_ctx *ctx, const uint8_t *keys, const uint32_t *key_lens, const uint32_t *path_lens, const int *ops,
                            const void *values, const uint32_t *value_lens, uint32_t n_preds, const uint8_t *program,
                            uint32_t program_len, uint64_t *count) {
    if (!ctx) return SJHIP_ERR_ARG;
    if (!count) {
        ctx_set_error(ctx, "sjhip_count_where_paths: a null count pointer");
        return SJHIP_ERR_ARG;
    }
    WhereMulti m;
    const int rc = where_multi_plan(ctx, "sjhip_count_where_paths", keys, key_lens, path_lens, ops, values, value_lens, n_preds, program,
                                    program_len, &m);
    if (rc) return rc;
    return count_over_parts(ctx, m.keys, m.klen, m.vals, m.vlen, true, count,
                            [&](sjhip_ctx *part, const QView &q, uint32_t n, unsigned long long *d) {
                                where_multi_launch(part, q, n, m.plan, QWhere(), d);
                            });
}

// ---- row predicates by membership in a set (sjhip_where_path_in, sjhip_count_where_path_in) ----------------------------------------
// The arguments of both calls are checked on the host -- nothing of the context is touched, nothing of the values is read before
// their number has been --; then every part that has rows gets the set in its d_in (uploaded as it came, the table cleared,
// k_q_in_build queued on the part's stream, in front of the mark that probes it), and the rest is where_build with k_q_in_mark, or
// the count.  The set is working data of the call: d_in is written over by the next one and freed by sjhip_ctx_trim.
struct InArgs {
    int kind;
    const uint64_t *offs;  // STRING
    const void *values;
    u32 n;
    size_t bytes;          // STRING: of all values
    QPath pth;
    const uint8_t *keys;
    size_t klen;
    u32 negate;
};
static int in_args(sjhip_ctx *ctx, const char *who, const uint8_t *keys, const uint32_t *key_lens, uint32_t n_keys, int kind,
                   const uint64_t *value_offsets, const void *values, size_t n_values, uint32_t flags, InArgs *a) {
    if (flags & ~SJHIP_WHERE_NOT) {
        ctx_set_error(ctx, "%s: unknown flag bits 0x%x", who, flags & ~SJHIP_WHERE_NOT);
        return SJHIP_ERR_ARG;
    }
    if (kind != SJHIP_COL_STRING && kind != SJHIP_COL_INT && kind != SJHIP_COL_UINT) {
        ctx_set_error(ctx, "%s: kind %d (a set holds SJHIP_COL_STRING, SJHIP_COL_INT or SJHIP_COL_UINT values)", who, kind);
        return SJHIP_ERR_ARG;
    }
    if (n_values > (size_t)SJHIP_WHERE_IN_MAX_VALUES) {
        ctx_set_error(ctx, "%s: %zu values (at most %u)", who, n_values, (unsigned)SJHIP_WHERE_IN_MAX_VALUES);
        return SJHIP_ERR_ARG;
    }
    a->kind = kind, a->offs = nullptr, a->values = values, a->n = (u32)n_values, a->bytes = 0, a->negate = flags & SJHIP_WHERE_NOT;
    if (kind == SJHIP_COL_STRING && n_values) {
        if (!value_offsets) {
            ctx_set_error(ctx, "%s: %zu string values are announced and `value_offsets` is null", who, n_values);
            return SJHIP_ERR_ARG;
        }
        if (value_offsets[0] != 0) {
            ctx_set_error(ctx, "%s: value_offsets[0] is %llu, not 0", who, (unsigned long long)value_offsets[0]);
            return SJHIP_ERR_ARG;
        }
        for (size_t j = 0; j < n_values; j++) {
            if (value_offsets[j + 1] < value_offsets[j]) {
                ctx_set_error(ctx, "%s: value_offsets[%zu] is smaller than the offset in front of it", who, j + 1);
                return SJHIP_ERR_ARG;
            }
            if (value_offsets[j + 1] - value_offsets[j] > (uint64_t)QMAX) {
                ctx_set_error(ctx, "%s: value %zu is %llu bytes long (a string value holds at most %d)", who, j,
                              (unsigned long long)(value_offsets[j + 1] - value_offsets[j]), QMAX);
                return SJHIP_ERR_ARG;
            }
        }
        a->offs = value_offsets;
        a->bytes = (size_t)value_offsets[n_values];
    }
    if (!values && (kind == SJHIP_COL_STRING ? a->bytes != 0 : n_values != 0)) {
        ctx_set_error(ctx, "%s: %zu values are announced and `values` is null", who, n_values);
        return SJHIP_ERR_ARG;
    }
    const int rc = make_path(ctx, keys, key_lens, n_keys, &a->pth, &a->klen, true);
    a->keys = keys ? keys : &NO_VALUE;
    return rc;
}
static size_t in_layout(Carve c, const InArgs &a, InSet *s) {
    const bool str = a.kind == SJHIP_COL_STRING;
    const size_t cap = (size_t)group_table_capacity(a.n), n_vals = (size_t)a.n + (str ? 1u : 0u);
    const u64 *const vals = c.take<u64>(n_vals);
    const u8 *const bytes = c.take<u8>(str ? a.bytes : 0);
    u64 *const hash = c.take<u64>(a.n);
    u32 *const table = c.take<u32>(cap);
    s->kind = a.kind, s->n = a.n, s->mask = (u32)(cap - 1);
    s->vals = SJ_ARR(vals, n_vals, A_IN_VALS);
    s->bytes = SJ_ARR(bytes, str ? a.bytes : 0, A_IN_BYTES);
    s->hash = SJ_ARR(hash, a.n, A_IN_HASH);
    s->table = SJ_ARR(table, cap, A_IN_TABLE);
    return c.used;
}
// the set of every part that has rows, in the part's d_in, its build queued on the part's stream; sets[k]: part k's (n == 0: none)
static int in_upload(sjhip_ctx *ctx, sjhip_ctx *part, const InArgs &a, InSet *s) {
    HIPCHK(hipSetDevice(part->device), "hipSetDevice");
    const int rc = reserve_layout(part, part->d_in, [&](Carve c) { return in_layout(c, a, s); });
    if (rc) return rc;
    const bool str = a.kind == SJHIP_COL_STRING;
    HIPCHK(hipMemcpyAsync((void *)arr_raw(s->vals), str ? (const void *)a.offs : a.values, ((size_t)a.n + (str ? 1u : 0u)) * 8,
                          hipMemcpyHostToDevice, part->stream), "H2D set values");
    if (str && a.bytes)
        HIPCHK(hipMemcpyAsync((void *)arr_raw(s->bytes), a.values, a.bytes, hipMemcpyHostToDevice, part->stream), "H2D set bytes");
    HIPCHK(hipMemsetAsync(arr_raw(s->table), 0xff, ((size_t)s->mask + 1u) * 4, part->stream), "set table memset");
    hipLaunchKernelGGL(k_q_in_build, dim3((a.n + 255) / 256), dim3(256), 0, part->stream, *s);
    HIPCHK(hipGetLastError(), "set build launch");
    return SJHIP_OK;
}
// the parts of either call: query_parts, and every part's result still on the device (make_view's check, made here before
// anything is uploaded)
static int in_parts(sjhip_ctx *ctx, const InArgs &a, std::vector<sjhip_ctx *> *parts) {
    const int rc = query_parts(ctx, a.keys, a.klen, &NO_VALUE, 0, parts);
    if (rc) return rc;
    for (const sjhip_ctx *part : *parts)
        if (!part->res.resident()) return no_result(ctx);
    return SJHIP_OK;
}
static int in_prepare(sjhip_ctx *ctx, const std::vector<sjhip_ctx *> &parts, const InArgs &a, std::vector<InSet> *sets) {
    sets->assign(parts.size(), InSet());
    int rc = SJHIP_OK;
    size_t k = 0;
    for (; k < parts.size() && rc == SJHIP_OK; k++)
        if (a.n && part_rows(ctx, parts[k], true)) rc = in_upload(ctx, parts[k], a, &(*sets)[k]);
    if (rc)  // (the copies read the caller's arrays: none is left in flight behind the return)
        for (size_t j = 0; j < k; j++)
            if (hipSetDevice(parts[j]->device) == hipSuccess) (void)hipStreamSynchronize(parts[j]->stream);
    (void)hipSetDevice(ctx->device);
    return rc;
}
static const InSet &in_set_of(const std::vector<sjhip_ctx *> &parts, const std::vector<InSet> &sets, const sjhip_ctx *part) {
    size_t k = 0;
    while (k + 1 < parts.size() && parts[k] != part) k++;
    return sets[k];
}
static void in_launch(sjhip_ctx *part, const QView &q, uint32_t n, const InArgs &a, const InSet &s, const QWhere &w, unsigned long long *count) {
    hipLaunchKernelGGL(k_q_in_mark, dim3((n + 255) / 256), dim3(256), 0, part->stream, q, a.pth, s, a.negate, w, count);
}

int sjhip_where_path_in(sjhip_ctx *ctx, const uint8_t *keys, const uint32_t *key_lens, uint32_t n_keys, int kind,
                        const uint64_t *value_offsets, const void *values, size_t n_values, uint32_t flags, size_t *records, size_t *rows) {
    if (!ctx) return SJHIP_ERR_ARG;
    if (!records || !rows) {
        ctx_set_error(ctx, "sjhip_where_path_in: a null size pointer");
        return SJHIP_ERR_ARG;
    }
    InArgs a;
    int rc = in_args(ctx, "sjhip_where_path_in", keys, key_lens, n_keys, kind, value_offsets, values, n_values, flags, &a);
    if (rc) return rc;
    std::vector<sjhip_ctx *> parts;
    rc = in_parts(ctx, a, &parts);
    if (rc) return rc;  // (nothing has been queued: the selection is as it was)
    std::vector<InSet> sets;
    rc = in_prepare(ctx, parts, a, &sets);
    if (rc == SJHIP_OK)
        rc = where_build(ctx, parts, a.keys, a.klen, &NO_VALUE, 0,
                         [&](sjhip_ctx *part, const QView &q, uint32_t n, const QWhere &w) {
                             in_launch(part, q, n, a, in_set_of(parts, sets, part), w, nullptr);
                         },
                         records, rows);
    return rc ? where_gave_up(ctx, parts, "sjhip_where_path_in", rc) : rc;
}

int sjhip_count_where_path_in(sjhip_ctx *ctx, const uint8_t *keys, const uint32_t *key_lens, uint32_t n_keys, int kind,
                              const uint64_t *value_offsets, const void *values, size_t n_values, uint32_t flags, uint64_t *count) {
    if (!ctx) return SJHIP_ERR_ARG;
    if (!count) {
        ctx_set_error(ctx, "sjhip_count_where_path_in: a null count pointer");
        return SJHIP_ERR_ARG;
    }
    InArgs a;
    int rc = in_args(ctx, "sjhip_count_where_path_in", keys, key_lens, n_keys, kind, value_offsets, values, n_values, flags, &a);
    if (rc) return rc;
    std::vector<sjhip_ctx *> parts;
    rc = in_parts(ctx, a, &parts);
    if (rc) return rc;
    std::vector<InSet> sets;
    rc = in_prepare(ctx, parts, a, &sets);
    if (rc) return rc;
    return count_over_parts(ctx, a.keys, a.klen, &NO_VALUE, 0, true, count,
                            [&](sjhip_ctx *part, const QView &q, uint32_t n, unsigned long long *d) {
                                in_launch(part, q, n, a, in_set_of(parts, sets, part), QWhere(), d);
                            });
}

// ---- unnest rows -------------------------------------------------------------------------------------------------------------------
// sjhip_unnest_rows replaces the selection of every part by the one a level further down and leaves the join back as a product of
// its own (d_parents, parents_layout).  Two passes over the parts, the shape of where_build / where_narrow: pass 1 runs on the old
// selection -- or, without one, on the records -- (make_view, on_rows) with its work arrays in d_kat: the parents' ranges, the depth
// prefix, the new rows counted (they come back through h_scratch + 512) and the new row offsets' room; pass 2 reserves d_parents
// for the counts and writes the new row index and parent[] there -- the old index is the input of that pass and the new selection
// may be larger than the arena the old one lies in, so the new index waits behind the product's arrays --, then reserves d_rows and
// copies offsets, statuses and index into it behind the kernels (stream order; a reservation that moves the arena waits for them).
struct ParentsOut { u64 *off, *parent, *new_index; u8 *status; };
static size_t parents_layout(Carve c, size_t parents, size_t rows, ParentsOut *o) {
    o->off = c.take<u64>(parents + 1);
    o->status = c.take<u8>(parents);
    o->parent = c.take<u64>(rows);
    o->new_index = c.take<u64>(rows);  // (on its way into d_rows: not part of what is fetched)
    return c.used;
}
struct UnnestWork {
    QUnnest u;
    u64 *new_off;             // [records + 1] the new row offsets
    u8 *new_status, *ok;      // [records] the statuses handed on; [records] all OK, what records without a selection hand on
    unsigned long long *totals;
};
static size_t unnest_layout(Carve c, const sjhip_ctx *part, uint32_t n, u32 depth_want, UnnestWork *w) {
    const u32 tiles = RowsBuild::tape_tiles(part);
    const size_t recs = (size_t)part->q_records + 1u;
    w->u.t = QRows{};
    w->totals = w->u.t.totals = c.take<unsigned long long>(32);
    u64 *const open = c.take<u64>(n), *const close = c.take<u64>(n);
    u8 *const status = c.take<u8>(n);
    w->u.open = SJ_ARR(open, n, A_UNNEST_RANGE);
    w->u.close = SJ_ARR(close, n, A_UNNEST_RANGE);
    w->u.status = SJ_ARR(status, n, A_UNNEST_STATUS);
    w->u.t.depth = c.take<unsigned long long>(tiles);
    w->u.t.cnt = c.take<unsigned long long>(tiles);
    w->u.t.tile_last = c.take<long long>(tiles);
    w->u.t.depth_want = depth_want;
    w->new_off = c.take<u64>(recs + 1);
    w->new_status = c.take<u8>(recs);
    w->ok = c.take<u8>(recs);
    return c.used;
}
// The walk of both calls on one part, in two halves, with nothing published -- sjhip_row_schema runs the same walk into its work
// arenas.  members: sjhip_unnest_members -- the parents' targets are objects and the tile passes are k_q_members_tile, whose counts are
// starts, two to a row; everything else is the same for both calls.
// unnest_count_enqueue: the parents' ranges, the depth prefix and the starts counted, on the work arrays `w` (unnest_layout); the
// count lies in w.totals[1] behind it.
static int unnest_count_enqueue(sjhip_ctx *ctx, sjhip_ctx *part, const QView &q, uint32_t n, const QPath &pth, bool members, const UnnestWork &w) {
    void (*const k_parents)(QView, QPath, QUnnest) = members ? k_q_members_parents : k_q_unnest_parents;
    void (*const k_count)(QView, QUnnest, Arr<u64>, Arr<u64>) = members ? k_q_members_tile<1> : k_q_unnest_tile<1>;
    const dim3 tiles(RowsBuild::tape_tiles(part)), block(TW_THREADS), one(1), wide(1024);
    unsigned long long *const none = nullptr;
    const Arr<u64> no_index = SJ_ARR((u64 *)nullptr, 0, A_ROWS), no_parent = SJ_ARR((u64 *)nullptr, 0, A_UNNEST_PARENT);
    HIPCHK(hipMemsetAsync(w.totals, 0, 256, part->stream), "unnest totals memset");
    hipLaunchKernelGGL(k_parents, dim3((n + 255) / 256), dim3(256), 0, part->stream, q, pth, w.u);
    hipLaunchKernelGGL(k_q_rows_tile<0>, tiles, block, 0, part->stream, q, w.u.t, 0u, no_index);
    hipLaunchKernelGGL(k_q_rows_last, tiles, block, 0, part->stream, q, w.u.t);  // (these three end at once unless a tile asked)
    hipLaunchKernelGGL(k_q_rows_scan_last, one, wide, 0, part->stream, w.u.t, tiles.x);
    hipLaunchKernelGGL(k_q_rows_tile<0>, tiles, block, 0, part->stream, q, w.u.t, 1u, no_index);
    hipLaunchKernelGGL(k_tw_scan_sums, one, wide, 0, part->stream, w.u.t.depth, none, none, tiles.x, w.totals);
    hipLaunchKernelGGL(k_count, tiles, block, 0, part->stream, q, w.u, no_index, no_parent);
    hipLaunchKernelGGL(k_tw_scan_sums, one, wide, 0, part->stream, none, w.u.t.cnt, none, tiles.x, w.totals);  // the rows: totals[1]
    HIPCHK(hipGetLastError(), "unnest launch");
    return SJHIP_OK;
}
// unnest_write_enqueue: the `got` new rows (members: the values) written, each with its parent
static void unnest_write_enqueue(sjhip_ctx *part, const QView &q, bool members, const UnnestWork &w, Arr<u64> index, Arr<u64> parent) {
    void (*const k_write)(QView, QUnnest, Arr<u64>, Arr<u64>) = members ? k_q_members_tile<2> : k_q_unnest_tile<2>;
    hipLaunchKernelGGL(k_write, dim3(RowsBuild::tape_tiles(part)), dim3(TW_THREADS), 0, part->stream, q, w.u, index, parent);
}
static int unnest_build(sjhip_ctx *ctx, const std::vector<sjhip_ctx *> &parts, const uint8_t *keys, size_t klen, const QPath &pth, bool members,
                        size_t *records, size_t *parents, size_t *rows) {
    const bool sel = selected(ctx, true);
    const u32 depth = (sel ? ctx->res.rows.sizes().depth : 0u) + pth.n + 1u;  // of the new rows below their record's root value
    std::vector<UnnestWork> work(parts.size());
    std::vector<size_t> found(parts.size(), 0);
    int rc = query_over_parts(ctx, parts, keys, klen, &NO_VALUE, 0, true, "unnest sync",
        [&](const sjhip_ctx *part, uint32_t n) {
            UnnestWork w;
            return unnest_layout(Carve(), part, n, depth, &w) + 64;
        },
        [&](size_t k, sjhip_ctx *part, const QView &q, uint32_t n) -> int {
            UnnestWork &w = work[k];
            (void)unnest_layout(Carve(part->d_kat.p), part, n, depth, &w);
            const int rc = unnest_count_enqueue(ctx, part, q, n, pth, members, w);
            if (rc) return rc;
            HIPCHK(hipMemcpyAsync(part->h_scratch + 512, w.totals + 1, 8, hipMemcpyDeviceToHost, part->stream), "D2H unnested row count");
            return SJHIP_OK;
        },
        [&](size_t k, sjhip_ctx *part) {
            found[k] = part_rows(ctx, part, true) ? (size_t)*(const unsigned long long *)(part->h_scratch + 512) : 0;
            if (members) found[k] /= 2;  // (the starts of a part: a key and a value for every member)
        });
    if (rc) return rc;
    rc = query_over_parts(ctx, parts, keys, klen, &NO_VALUE, 0, true, "unnest gather sync", [](const sjhip_ctx *, uint32_t) { return (size_t)0; },
        [&](size_t k, sjhip_ctx *part, const QView &q, uint32_t n) -> int {
            const UnnestWork &w = work[k];
            const size_t recs = (size_t)part->q_records + 1u, got = found[k];
            ParentsOut po;
            int rc = reserve_layout(part, part->d_parents, [&](Carve cv) { return parents_layout(cv, n, got, &po); });
            if (rc) return rc;
            const Arr<const u64> index = SJ_ARR((const u64 *)po.new_index, got, A_ROWS);
            if (got) unnest_write_enqueue(part, q, members, w, SJ_ARR(po.new_index, got, A_ROWS), SJ_ARR(po.parent, got, A_UNNEST_PARENT));
            // the records: their new offsets, and the status bytes they had (without a selection: OK)
            QRows hand = w.u.t;
            hand.status = w.ok;
            if (sel) {
                const ResultState::Rows &z = part->res.rows.sizes();
                RowsOut old;
                (void)rows_layout(Carve(part->d_rows.p), z.records, z.rows, &old);
                hand.status = old.status;
            } else {
                HIPCHK(hipMemsetAsync(w.ok, SJHIP_COL_OK, recs, part->stream), "unnest status memset");
            }
            hipLaunchKernelGGL(k_q_rows_offsets, dim3(((u32)recs + 255) / 256), dim3(256), 0, part->stream, q, hand, index, (u64)got, w.new_off,
                               w.new_status);
            hipLaunchKernelGGL(k_q_unnest_offsets, dim3((n + 1u + 255) / 256), dim3(256), 0, part->stream, q, w.u, index, (u64)got,
                               SJ_ARR(po.off, (size_t)n + 1, A_UNNEST_OFF), SJ_ARR(po.status, n, A_UNNEST_STATUS));
            HIPCHK(hipGetLastError(), "unnest gather launch");
            RowsOut o;
            rc = reserve_layout(part, part->d_rows, [&](Carve cv) { return rows_layout(cv, recs, got, &o); });
            if (rc) return rc;
            HIPCHK(hipMemcpyAsync(o.off, w.new_off, (recs + 1) * 8, hipMemcpyDeviceToDevice, part->stream), "row offsets copy");
            HIPCHK(hipMemcpyAsync(o.status, w.new_status, recs, hipMemcpyDeviceToDevice, part->stream), "row status copy");
            if (got) HIPCHK(hipMemcpyAsync(o.index, po.new_index, got * 8, hipMemcpyDeviceToDevice, part->stream), "row index copy");
            return SJHIP_OK;
        },
        [](size_t, sjhip_ctx *) {});
    if (rc) return rc;
    ResultState::Rows total;
    ResultState::Parents joined;
    total.depth = depth;
    total.members = members;
    bool ok = true;  // (a part without parents launched nothing: its selection, no rows, keeps its offsets and statuses)
    for (size_t k = 0; k < parts.size(); k++) {
        const ResultState::Rows s = {(size_t)parts[k]->q_records + 1u, found[k], depth, members};
        const ResultState::Parents p = {(size_t)part_rows(ctx, parts[k], true), found[k]};
        total.records += s.records, total.rows += s.rows;
        joined.parents += p.parents, joined.rows += p.rows;
        ok &= parts[k]->res.publish(&ResultState::rows, s) && parts[k]->res.publish(&ResultState::parents, p);
    }
    if (ctx->res.sharded()) ok &= ctx->res.publish(&ResultState::rows, total) && ctx->res.publish(&ResultState::parents, joined);
    *records = total.records, *parents = joined.parents, *rows = total.rows;
    return published(ctx, ok);
}

// sjhip_unnest_rows and sjhip_unnest_members (`who`): the checks, which touch nothing, then the build
static int unnest_entry(sjhip_ctx *ctx, const char *who, bool members, const uint8_t *keys, const uint32_t *key_lens, uint32_t n_keys,
                        size_t *records, size_t *parents, size_t *rows) {
    if (!ctx) return SJHIP_ERR_ARG;
    if (!records || !parents || !rows) {
        ctx_set_error(ctx, "%s: a null size pointer", who);
        return SJHIP_ERR_ARG;
    }
    QPath pth;
    size_t klen = 0;
    int rc = make_path(ctx, keys, key_lens, n_keys, &pth, &klen, true);
    if (rc) return rc;
    const uint8_t *const kb = keys ? keys : &NO_VALUE;
    std::vector<sjhip_ctx *> parts;
    rc = query_parts(ctx, kb, klen, &NO_VALUE, 0, &parts);
    if (rc) return rc;
    // ---- nothing was touched up to here; from here on the last parents product is gone ----
    ctx->res.parents.begin();
    for (sjhip_ctx *part : parts) part->res.parents.begin();
    rc = unnest_build(ctx, parts, kb, klen, pth, members, records, parents, rows);
    if (rc) {  // half-built: the old selection may have been written over
        ctx->res.rows.begin(), ctx->res.parents.begin();
        for (sjhip_ctx *part : parts) part->res.rows.begin(), part->res.parents.begin();
        char why[sizeof ctx->err];
        snprintf(why, sizeof why, "%s", ctx->err);
        ctx_set_error(ctx, "%s failed, the row selection was given up and no row parents are left: %.160s", who, why);
    }
    return rc;
}
int sjhip_unnest_rows(sjhip_ctx *ctx, const uint8_t *keys, const uint32_t *key_lens, uint32_t n_keys, size_t *records, size_t *parents,
                      size_t *rows) {
    return unnest_entry(ctx, "sjhip_unnest_rows", false, keys, key_lens, n_keys, records, parents, rows);
}
int sjhip_unnest_members(sjhip_ctx *ctx, const uint8_t *keys, const uint32_t *key_lens, uint32_t n_keys, size_t *records, size_t *parents,
                         size_t *rows) {
    return unnest_entry(ctx, "sjhip_unnest_members", true, keys, key_lens, n_keys, records, parents, rows);
}

// ---- the names of member rows ------------------------------------------------------------------------------------------------------
// Both calls need the selection in force to be one of object members (ResultState::Rows::members: sjhip_unnest_members and every
// narrowing of what it left); the check comes first and touches nothing.
static int need_member_rows(sjhip_ctx *ctx) {
    if (ctx->res.member_rows()) return SJHIP_OK;
    ctx_set_error(ctx, "the rows in force are not object members (sjhip_extract_row_names follows sjhip_unnest_members)");
    return SJHIP_ERR_ARG;
}
int sjhip_extract_row_names(sjhip_ctx *ctx, size_t *records, size_t *bytes) {
    if (!ctx || !records || !bytes) return SJHIP_ERR_ARG;
    if (need_member_rows(ctx)) return SJHIP_ERR_ARG;
    ColumnBuild p;
    p.pth = QPath{}, p.cvt = 0, p.records = records, p.bytes = bytes, p.names = true;
    return build_product(ctx, &NO_VALUE, 0, p);
}
int sjhip_where_row_names(sjhip_ctx *ctx, int op, const void *value, size_t vlen, uint32_t flags, size_t *records, size_t *rows) {
    if (!ctx || !records || !rows) return SJHIP_ERR_ARG;
    if (flags & ~SJHIP_WHERE_NOT) {
        ctx_set_error(ctx, "sjhip_where_row_names: unknown flag bits 0x%x", flags & ~SJHIP_WHERE_NOT);
        return SJHIP_ERR_ARG;
    }
    bool is_str = false;
    u64 want = 0;
    if ((op != SJHIP_OP_EQ_STRING && op != SJHIP_OP_PREFIX_STRING) || predicate_value(op, value, vlen, &want, &is_str)) {
        ctx_set_error(ctx, "sjhip_where_row_names: operator %d with a value of %zu bytes (a name is a string: SJHIP_OP_EQ_STRING, SJHIP_OP_PREFIX_STRING)", op, vlen);
        return SJHIP_ERR_ARG;
    }
    if (need_member_rows(ctx)) return SJHIP_ERR_ARG;
    const uint8_t *const vb = value ? (const uint8_t *)value : &NO_VALUE;
    std::vector<sjhip_ctx *> parts;
    int rc = query_parts(ctx, &NO_VALUE, 0, vb, vlen, &parts);
    if (rc) return rc;  // (nothing has been queued: the selection is as it was)
    const u32 negate = flags & SJHIP_WHERE_NOT;
    rc = where_build(ctx, parts, &NO_VALUE, 0, vb, vlen,
                     [&](sjhip_ctx *part, const QView &q, uint32_t n, const QWhere &w) {
                         hipLaunchKernelGGL(k_q_names_mark, dim3((n + 255) / 256), dim3(256), 0, part->stream, q, op, want, negate, w);
                     },
                     records, rows);
    return rc ? where_gave_up(ctx, parts, "sjhip_where_row_names", rc) : rc;
}

int sjhip_fetch_row_parents(sjhip_ctx *ctx, uint64_t *parent_offsets, uint64_t *parent, uint8_t *parent_status) {
    if (!ctx) return SJHIP_ERR_ARG;
    if (!ctx->res.parents.exists())
        return no_product(ctx, "no row parents on the device (sjhip_fetch_row_parents follows sjhip_unnest_rows, with no parse in between)");
    // (RECORDS counts the parents here, ELEMS the new rows; parent[] counts in parents but has no terminating entry)
    const Seg segs[] = {{parent_offsets, 8, RECORDS, ELEMS, "D2H parent offsets"},
                        {parent_status, 1, RECORDS, NO_DOM, "D2H parent status"},
                        {parent, 8, ELEMS, RECORDS, "D2H row parents", false}};
    const int rc = fetch_joined(ctx, "row parents fetch sync", segs, 3,
        [](sjhip_ctx *part, size_t *count, const void **src) {
            const ResultState::Parents &s = part->res.parents.sizes();
            ParentsOut o;
            (void)parents_layout(Carve(part->d_parents.p), s.parents, s.rows, &o);
            count[RECORDS] = s.parents, count[ELEMS] = s.rows;
            src[0] = o.off, src[1] = o.status, src[2] = o.parent;
        },
        [](const size_t *) { return SJHIP_OK; });  // (any destination may be null: that array is not copied)
    return rc ? rc : query_bounds_check(ctx);  // (debug build: the kernels of sjhip_unnest_rows have finished here)
}

// ---- filter rows -------------------------------------------------------------------------------------------------------------------
// sjhip_filter_rows materialises the selection in force as the Filtered tenant of the shared arenas, in sjhip_filter_where's
// order: the checks (which touch nothing), the claim, the work arrays in d_q, measure and scan, the totals, the output arenas --
// sized from the measured totals: a row of two words becomes a record of four, the result can be larger than the tape it came
// from --, the publish, the copy.  It reads the selection and leaves it, and every other product, as they are.
int sjhip_filter_rows(sjhip_ctx *ctx, uint64_t *n_rows, uint64_t *skipped, size_t *tape_len, size_t *strings_len) {
    if (!ctx) return SJHIP_ERR_ARG;
    if (!ctx->res.whole()) return no_whole_result(ctx, "sjhip_filter_rows", "queries follow");  // the unsharded result of ctx itself
    if (!ctx->res.rows.exists())
        return no_product(ctx, "no row selection on the device (sjhip_filter_rows follows sjhip_select_rows or sjhip_where_path)");
    if (!(ctx->p_flags & SJHIP_FLAG_COPY_STRINGS)) {
        ctx_set_error(ctx, "sjhip_filter_rows needs a parse with SJHIP_FLAG_COPY_STRINGS (the filtered Strings.B is self-contained)");
        return SJHIP_ERR_ARG;
    }
    QView q;
    int rc = make_view(ctx, ctx, &NO_VALUE, 0, &NO_VALUE, 0, &q, true);
    if (rc) return rc;
    const uint32_t n = part_rows(ctx, ctx, true);
    HIPCHK(hipSetDevice(ctx->device), "hipSetDevice");
    ctx->res.claim_shared();
    unsigned long long *h = (unsigned long long *)(ctx->h_scratch + 512);
    memset(h, 0, 48);  // (a selection without rows measures nothing)
    QFRows o{};
    if (n) {
        const u32 tiles = (n + QTILE - 1) / QTILE;
        rc = reserve_layout(ctx, ctx->d_q, [&](Carve c) {
            o.totals = c.take<unsigned long long>(32);
            u32 *const words = c.take<u32>(n), *const first_str = c.take<u32>(n), *const s_len = c.take<u32>(n), *const s_pre = c.take<u32>(n);
            o.words = SJ_ARR(words, n, A_FROWS_WORDS);
            o.first_str = SJ_ARR(first_str, n, A_FROWS_STR);
            o.s_len = SJ_ARR(s_len, n, A_FROWS_STR);
            o.s_pre = SJ_ARR(s_pre, n, A_FROWS_STR);
            o.tw = c.take<unsigned long long>(tiles);
            o.tb = c.take<unsigned long long>(tiles);
            return c.used;
        });
        if (rc) return rc;
        unsigned long long *const none = nullptr;
        HIPCHK(hipMemsetAsync(o.totals, 0, 256, ctx->stream), "filter rows totals memset");
        hipLaunchKernelGGL(k_q_frows_measure, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, q, o);
        hipLaunchKernelGGL(k_q_frows_tile_sums, dim3(tiles), dim3(QT), 0, ctx->stream, o, n);
        hipLaunchKernelGGL(k_tw_scan_sums, dim3(1), dim3(1024), 0, ctx->stream, o.tw, o.tb, none, tiles, o.totals);
        hipLaunchKernelGGL(k_q_frows_tile_apply, dim3(tiles), dim3(QT), 0, ctx->stream, o, n);
        HIPCHK(hipGetLastError(), "filter rows launch");
        HIPCHK(hipMemcpyAsync(h, o.totals, 48, hipMemcpyDeviceToHost, ctx->stream), "D2H filter rows totals");
        HIPCHK(hipStreamSynchronize(ctx->stream), "filter rows sync");
    }
    const unsigned long long words = h[0], bytes = h[1], emitted = h[4], scalars = h[5];  // (sums of 64 bits)
    if (words > 0xffffffffull) {
        ctx_set_error(ctx, "sjhip_filter_rows: the result would hold %llu tape words (at most 2^32 - 1)", words);
        return SJHIP_ERR_TOOBIG;
    }
    if (emitted) {
        rc = arena_reserve(ctx, ctx->d_qtape, (size_t)words * 8 + 64);
        if (rc) return rc;
        rc = arena_reserve(ctx, ctx->d_qstrings, (size_t)bytes + 64);
        if (rc) return rc;
    }
    rc = published(ctx, ctx->res.publish_filtered({(size_t)words, (size_t)bytes}));
    if (rc) return rc;
    if (n_rows) *n_rows = emitted;
    if (skipped) *skipped = scalars;
    if (tape_len) *tape_len = (size_t)words;
    if (strings_len) *strings_len = (size_t)bytes;
    if (emitted == 0) return query_bounds_check(ctx);
    hipLaunchKernelGGL(k_q_frows_copy, dim3((n + 3) / 4), dim3(256), 0, ctx->stream, q, o, SJ_ARR((u64 *)ctx->d_qtape.p, words, A_FROWS_TAPE),
                       SJ_ARR((u8 *)ctx->d_qstrings.p, bytes, A_FROWS_STRINGS));
    HIPCHK(hipGetLastError(), "filter rows copy launch");
    return SJHIP_OK;
}

// ---- queries on the whole result of one context (groups, order) ----------------------------------------------------------------------
// The checks both run behind their own arguments, in this order and with nothing touched: the paths; a sharded result refused
// (`unjoined`: what would have to be done across shards); a whole result; the views of the rows in force; at most 2^30 rows (*n).
struct WholePath {
    const uint8_t *keys;  // in: the call's keys (null: no keys, the row's own value)
    const uint32_t *key_lens;
    uint32_t n_keys;
    QPath pth;            // out
    size_t klen;
    QView q;
};
static int whole_entry(sjhip_ctx *ctx, const char *call, const char *unjoined, WholePath *paths, int n_paths, uint32_t *n) {
    int rc = SJHIP_OK;
    for (int k = 0; k < n_paths && !rc; k++) rc = make_path(ctx, paths[k].keys, paths[k].key_lens, paths[k].n_keys, &paths[k].pth, &paths[k].klen, true);
    if (rc) return rc;
    if (ctx->res.sharded()) {
        ctx_set_error(ctx, "%s: the result is sharded (an ND message beyond one context's reach); %s", call, unjoined);
        return SJHIP_ERR_ARG;
    }
    if (!ctx->res.whole()) return no_whole_result(ctx, call, "queries follow");
    for (int k = 0; k < n_paths && !rc; k++) {
        if (!paths[k].keys) paths[k].keys = &NO_VALUE;
        rc = make_view(ctx, ctx, paths[k].keys, paths[k].klen, &NO_VALUE, 0, &paths[k].q, true);
    }
    if (rc) return rc;
    *n = part_rows(ctx, ctx, true);
    if (*n > (1u << 30)) {
        ctx_set_error(ctx, "%s: %u rows (at most 2^30)", call, *n);
        return SJHIP_ERR_TOOBIG;
    }
    return SJHIP_OK;
}
// the D2H copies of a fetch on the context's stream, then one wait; a null destination and an empty array are skipped
struct FetchCopy { void *dst; const void *src; size_t bytes; };
static int fetch_copies(sjhip_ctx *ctx, const FetchCopy *copies, size_t n, const char *copy_what, const char *sync_what) {
    HIPCHK(hipSetDevice(ctx->device), "hipSetDevice");
    for (size_t k = 0; k < n; k++)
        if (copies[k].dst && copies[k].bytes)
            HIPCHK(hipMemcpyAsync(copies[k].dst, copies[k].src, copies[k].bytes, hipMemcpyDeviceToHost, ctx->stream), copy_what);
    HIPCHK(hipStreamSynchronize(ctx->stream), sync_what);
    return SJHIP_OK;
}

// ---- groups --------------------------------------------------------------------------------------------------------------------------
// sjhip_group_path and sjhip_group_paths work on the whole result of one context (a sharded one is refused: its dictionaries would
// have to be joined); each checks its own arguments and hands over to group_build.  The work arrays of all the kernels (GroupWork)
// lie in d_kat, laid out once for the row count and the columns -- the group count is only known after the first half, and a second
// reservation would move the arena --; the product (group_layout: per key column its entries and statuses, per value column six
// aggregate arrays) lies in d_group, reserved when the scans have told the groups and every STRING column's key bytes.  One host
// round trip in the middle (those totals and the rows in a group), one wait at the end.
// Behind the emit of a grouping, by one key or by several: the n rows ordered by code, stably (the first pass's keys lie in
// sort.keys[0]); the offsets and sizes of the G groups over the n_in sorted rows that are in a group; and one segmented reduction
// per value column over those rows -- groups in the place of records, on the work arrays `laid` out for n rows.
struct GroupValue {
    const QView *q;
    const QPath *pth;
    int kind;
    u64 *out;  // [6 * G] in the product
};
static int group_reduce(sjhip_ctx *ctx, uint32_t n, u32 n_in, u32 G, const SortWork<u32> &sort, u64 *off, Arr<u64> group_rows,
                        const AggWork &laid, const GroupValue *vals, uint32_t n_vals) {
    if (!G) return SJHIP_OK;
    hipStream_t st = ctx->stream;
    const dim3 b256(256);
    const int at = sort_enqueue(st, n, n, group_pass_mask(G), false, sort);
    const u32 *const skeys = sort.keys[at], *const srows = sort.rows[at];
    hipLaunchKernelGGL(k_q_group_bounds, dim3((n_in + 255) / 256), b256, 0, st, SJ_ARR(skeys, n, A_SORT), n_in, G,
                       SJ_ARR(off, (size_t)G + 1, A_GROUP_OFF));
    hipLaunchKernelGGL(k_q_group_counts, dim3((G + 255) / 256), b256, 0, st, SJ_ARR((const u64 *)off, (size_t)G + 1, A_GROUP_OFF), G, group_rows);
    HIPCHK(hipGetLastError(), "group sort launch");
    for (uint32_t v = 0; v < n_vals; v++) {
        AggWork aw;
        (void)agg_layout(Carve(), n_in, G, AGG_OFFS, &aw, false);  // (the levels of n_in rows; the arrays: those laid out for n)
        aw.out = vals[v].out;
        aw.head = laid.head;
        for (size_t l = 0; l < aw.items.size(); l++) aw.items[l] = laid.items[l];
        const int rc = agg_enqueue(ctx, ctx, *vals[v].q, *vals[v].pth, vals[v].kind, AGG_OFFS, n_in, G, off, aw, srows);
        if (rc) return rc;
    }
    return SJHIP_OK;
}
struct GroupWork {
    unsigned long long *totals;  // [0] groups, [2] rows in a group; the key bytes of the length array s: [1] for s = 0, else [2 + s]
    QGroup g;
    SortWork<u32> sort;
    u64 *off;  // [groups + 1] the group offsets in the sorted order (room for one group per row)
    AggWork agg;
};
static size_t group_work_layout(Carve c, uint32_t n, const int *kinds, const uint32_t *flags, uint32_t n_cols, bool value, GroupWork *w) {
    const u64 cap = group_table_capacity(n);
    const u32 tiles = tiles_of(n);
    QGroup &g = w->g;
    w->totals = c.take<unsigned long long>(32);
    g.n = n, g.mask = (u32)(cap - 1), g.n_cols = n_cols, g.tiles = tiles;
    g.kinds = g.null_mask = g.str_slot = 0;
    u32 n_str = 0;
    for (u32 k = 0; k < n_cols; k++) {
        g.kinds |= (u32)kinds[k] << (4 * k);
        if (flags && (flags[k] & SJHIP_GROUP_NULL_KEY)) g.null_mask |= 1u << k;
        if (kinds[k] == SJHIP_COL_STRING) g.str_slot |= n_str++ << (4 * k);
    }
    const size_t per_col = (size_t)n_cols * n, lens = (size_t)n_str * ((size_t)n + 1);
    u8 *const status = c.take<u8>(per_col), *const in = c.take<u8>(n);
    u64 *const kidx = c.take<u64>(per_col), *const hash = c.take<u64>(n);
    u32 *const slot = c.take<u32>(n), *const table = c.take<u32>(cap), *const flag = c.take<u32>((size_t)n + 1);
    u64 *const len = n_str ? c.take<u64>(lens) : nullptr;
    g.status = SJ_ARR(status, per_col, A_GROUP_ROW);
    g.in = SJ_ARR(in, n, A_GROUP_ROW);
    g.kidx = SJ_ARR(kidx, per_col, A_GROUP_ROW);
    g.hash = SJ_ARR(hash, n, A_GROUP_ROW);
    g.slot = SJ_ARR(slot, n, A_GROUP_ROW);
    g.table = SJ_ARR(table, cap, A_GROUP_TABLE);
    g.flag = SJ_ARR(flag, (size_t)n + 1, A_GROUP_ROW);
    g.len = SJ_ARR(len, lens, A_GROUP_LEN);
    g.tiles_f = c.take<unsigned long long>(tiles);
    g.tiles_o = c.take<unsigned long long>(tiles);
    g.tiles_l = c.take<unsigned long long>((size_t)n_str * tiles);
    sort_carve(c, n, &w->sort);
    w->off = c.take<u64>((size_t)n + 1);
    if (value) (void)(c.used = agg_layout(c, n, n, AGG_OFFS, &w->agg, false));
    return c.used;
}
// The grouping in d_group: what the fetches return, and nothing else.
struct GroupArrays {
    u64 *first_row, *group_rows, *agg[ResultState::GROUP_COLS], *key_off[ResultState::GROUP_COLS], *key_val[ResultState::GROUP_COLS];
    u32 *codes;
    u8 *key_bytes[ResultState::GROUP_COLS], *key_u8[ResultState::GROUP_COLS], *key_ok[ResultState::GROUP_COLS], *status[ResultState::GROUP_COLS];
};
static size_t group_layout(Carve c, const ResultState::Groups &z, GroupArrays *o) {
    *o = GroupArrays{};
    o->first_row = c.take<u64>(z.groups);
    o->group_rows = c.take<u64>(z.groups);
    for (uint32_t v = 0; v < z.val_cols; v++) o->agg[v] = c.take<u64>(6 * z.groups);
    for (uint32_t k = 0; k < z.key_cols; k++) {
        if (z.key_kinds[k] == SJHIP_COL_STRING) o->key_off[k] = c.take<u64>(z.groups + 1);
        else if (z.key_kinds[k] != SJHIP_COL_BOOL) o->key_val[k] = c.take<u64>(z.groups);
    }
    o->codes = c.take<u32>(z.rows);
    for (uint32_t k = 0; k < z.key_cols; k++) {
        if (z.key_kinds[k] == SJHIP_COL_STRING) o->key_bytes[k] = c.take<u8>(z.col_bytes[k]);
        else if (z.key_kinds[k] == SJHIP_COL_BOOL) o->key_u8[k] = c.take<u8>(z.groups);
        o->key_ok[k] = c.take<u8>(z.groups);
        o->status[k] = c.take<u8>(z.rows);
    }
    return c.used;
}
// The build behind the argument checks of both calls (`call` names the caller in the error texts): k holds the paths of the
// n_key_cols key columns, then those of the n_val_cols value columns; key_flags may be null (no column has a flag).
static int group_build(sjhip_ctx *ctx, const char *call, WholePath *k, const int *key_kinds, const uint32_t *key_flags, uint32_t n_key_cols,
                       const int *val_kinds, uint32_t n_val_cols, size_t *rows, size_t *groups, size_t *key_bytes) {
    uint32_t n = 0;
    int rc = whole_entry(ctx, call, "the dictionaries of shards are not joined", k, (int)(n_key_cols + n_val_cols), &n);
    if (rc) return rc;
    // ---- nothing was touched up to here; from here on the last grouping is gone ----
    ctx->res.groups.begin();
    ResultState::Groups z;
    z.rows = n, z.key_cols = n_key_cols, z.val_cols = n_val_cols;
    for (uint32_t c = 0; c < n_key_cols; c++) z.key_kinds[c] = key_kinds[c], key_bytes[c] = 0;
    for (uint32_t v = 0; v < n_val_cols; v++) z.val_kinds[v] = val_kinds[v];
    HIPCHK(hipSetDevice(ctx->device), "hipSetDevice");
    if (n == 0) {
        *rows = *groups = 0;
        return published(ctx, ctx->res.publish(&ResultState::groups, z));
    }
    GroupWork w;
    rc = reserve_layout(ctx, ctx->d_kat, [&](Carve c) { return group_work_layout(c, n, key_kinds, key_flags, n_key_cols, n_val_cols != 0, &w); });
    if (rc) return rc;
    const QView &q0 = k[0].q;  // (the kernels behind the walks read the tape and the strings only: any column's view)
    hipStream_t st = ctx->stream;
    const dim3 per_row((n + 255) / 256), per_entry((n + 1u + 255) / 256), b256(256), one(1), wide(1024);
    unsigned long long *const none = nullptr;
    const u32 tiles = w.g.tiles;
    u32 n_str = 0;
    for (uint32_t c = 0; c < n_key_cols; c++) n_str += key_kinds[c] == SJHIP_COL_STRING;
    HIPCHK(hipMemsetAsync(w.totals, 0, 256, st), "group totals memset");
    HIPCHK(hipMemsetAsync(arr_raw(w.g.table), 0xff, ((size_t)w.g.mask + 1) * 4, st), "group table memset");
    for (uint32_t c = 0; c < n_key_cols; c++) hipLaunchKernelGGL(k_q_group_keys, per_row, b256, 0, st, k[c].q, k[c].pth, w.g, c);
    hipLaunchKernelGGL(k_q_group_insert, per_row, b256, 0, st, q0, w.g);
    hipLaunchKernelGGL(k_q_group_first, per_entry, b256, 0, st, q0, w.g);
    // sums -> scan -> apply: the flags with the length array 0 beside them, then one round per further length array
    for (u32 round = 0; round == 0 || round < n_str; round++) {
        hipLaunchKernelGGL(k_q_group_tile_sums, dim3(tiles), dim3(QT), 0, st, w.g, n + 1u, round);
        if (round == 0) hipLaunchKernelGGL(k_tw_scan_sums, one, wide, 0, st, w.g.tiles_f, n_str ? w.g.tiles_l : none, w.g.tiles_o, tiles, w.totals);
        else hipLaunchKernelGGL(k_tw_scan_sums, one, wide, 0, st, w.g.tiles_l + (size_t)round * tiles, none, none, tiles, w.totals + 2 + round);
        hipLaunchKernelGGL(k_q_group_tile_apply, dim3(tiles), dim3(QT), 0, st, w.g, n + 1u, round);
    }
    HIPCHK(hipGetLastError(), "group launch");
    unsigned long long *const h = (unsigned long long *)(ctx->h_scratch + 512);
    HIPCHK(hipMemcpyAsync(h, w.totals, (3 + (size_t)ResultState::GROUP_COLS) * 8, hipMemcpyDeviceToHost, st), "D2H group totals");
    HIPCHK(hipStreamSynchronize(st), "group sync");
    rc = query_bounds_check(ctx);
    if (rc) return rc;
    const u32 G = (u32)h[0], n_in = (u32)h[2];
    z.groups = G;
    for (uint32_t c = 0, s = 0; c < n_key_cols; c++) {
        const int kind = key_kinds[c];
        if (kind != SJHIP_COL_STRING) z.col_bytes[c] = kind == SJHIP_COL_BOOL ? (size_t)G : (size_t)8 * G;
        else z.col_bytes[c] = (size_t)h[s ? 2 + s : 1], s++;
    }
    GroupArrays a;
    rc = reserve_layout(ctx, ctx->d_group, [&](Carve c) { return group_layout(c, z, &a); });
    if (rc) return rc;
    u32 *const first_keys = w.sort.keys[0];
    for (uint32_t c = 0; c < n_key_cols; c++) {
        GroupOut o;
        u64 *const key_off = a.key_off[c], *const key_val = a.key_val[c];
        u8 *const col_bytes = a.key_bytes[c], *const key_u8 = a.key_u8[c], *const key_ok = a.key_ok[c], *const status = a.status[c];
        o.key_off = SJ_ARR(key_off, key_off ? (size_t)G + 1 : 0, A_GROUP_OUT);
        o.key_bytes = SJ_ARR(col_bytes, col_bytes ? z.col_bytes[c] : 0, A_GROUP_KEYS);
        o.key_val = SJ_ARR(key_val, key_val ? G : 0, A_GROUP_OUT);
        o.key_u8 = SJ_ARR(key_u8, key_u8 ? G : 0, A_GROUP_OUT);
        o.key_ok = SJ_ARR(key_ok, G, A_GROUP_OUT);
        o.status = SJ_ARR(status, n, A_GROUP_OUT);
        o.first_row = SJ_ARR(a.first_row, G, A_GROUP_OUT);
        o.codes = SJ_ARR(a.codes, n, A_GROUP_OUT);
        hipLaunchKernelGGL(k_q_group_emit, per_row, b256, 0, st, q0, w.g, o, G, SJ_ARR(first_keys, n, A_SORT), c);
    }
    GroupValue gv[ResultState::GROUP_COLS];
    for (uint32_t v = 0; v < n_val_cols; v++) gv[v] = {&k[n_key_cols + v].q, &k[n_key_cols + v].pth, val_kinds[v], a.agg[v]};
    rc = group_reduce(ctx, n, n_in, G, w.sort, w.off, SJ_ARR(a.group_rows, G, A_GROUP_OUT), w.agg, gv, n_val_cols);
    if (rc) return rc;
    HIPCHK(hipGetLastError(), "group emit launch");
    HIPCHK(hipStreamSynchronize(st), "group build sync");
    rc = query_bounds_check(ctx);
    if (rc) return rc;
    *rows = n, *groups = G;
    for (uint32_t c = 0; c < n_key_cols; c++) key_bytes[c] = z.col_bytes[c];
    return published(ctx, ctx->res.publish(&ResultState::groups, z));
}

int sjhip_group_paths(sjhip_ctx *ctx, const uint8_t *keys, const uint32_t *key_lens, const uint32_t *key_path_lens, const int *key_kinds,
                      const uint32_t *key_flags, uint32_t n_key_cols, const uint32_t *val_path_lens, const int *val_kinds,
                      uint32_t n_val_cols, size_t *rows, size_t *groups, size_t *key_bytes) {
    if (!ctx) return SJHIP_ERR_ARG;
    if (!rows || !groups || !key_bytes) {
        ctx_set_error(ctx, "sjhip_group_paths: a null size pointer");
        return SJHIP_ERR_ARG;
    }
    if (n_key_cols < 1 || n_key_cols > (uint32_t)SJHIP_GROUP_MAX_KEYS) {
        ctx_set_error(ctx, "sjhip_group_paths: %u key columns (1 to %d)", n_key_cols, SJHIP_GROUP_MAX_KEYS);
        return SJHIP_ERR_ARG;
    }
    if (n_val_cols > (uint32_t)SJHIP_GROUP_MAX_VALUES) {
        ctx_set_error(ctx, "sjhip_group_paths: %u value columns (0 to %d)", n_val_cols, SJHIP_GROUP_MAX_VALUES);
        return SJHIP_ERR_ARG;
    }
    if (!key_path_lens || !key_kinds || (n_val_cols && (!val_path_lens || !val_kinds))) {
        ctx_set_error(ctx, "sjhip_group_paths: a null argument (key_path_lens, key_kinds, val_path_lens, val_kinds)");
        return SJHIP_ERR_ARG;
    }
    const uint32_t n_paths = n_key_cols + n_val_cols;
    size_t n_keys = 0, bytes = 0;
    for (uint32_t c = 0; c < n_paths; c++) {
        const bool is_key = c < n_key_cols;
        const uint32_t j = is_key ? c : c - n_key_cols;
        const int kind = is_key ? key_kinds[j] : val_kinds[j];
        if (is_key && kind != SJHIP_COL_STRING && kind != SJHIP_COL_INT && kind != SJHIP_COL_UINT && kind != SJHIP_COL_BOOL) {
            ctx_set_error(ctx, "sjhip_group_paths: key column %u: kind %d is not SJHIP_COL_STRING, SJHIP_COL_INT, SJHIP_COL_UINT or SJHIP_COL_BOOL", j,
                          kind);
            return SJHIP_ERR_ARG;
        }
        if (!is_key && kind != SJHIP_COL_FLOAT && kind != SJHIP_COL_INT && kind != SJHIP_COL_UINT) {
            ctx_set_error(ctx, "sjhip_group_paths: value column %u: kind %d is not SJHIP_COL_FLOAT, SJHIP_COL_INT or SJHIP_COL_UINT", j, kind);
            return SJHIP_ERR_ARG;
        }
        if (is_key && key_flags && (key_flags[j] & ~SJHIP_GROUP_NULL_KEY)) {
            ctx_set_error(ctx, "sjhip_group_paths: key column %u: unknown flag bits 0x%x", j, key_flags[j] & ~SJHIP_GROUP_NULL_KEY);
            return SJHIP_ERR_ARG;
        }
        n_keys += is_key ? key_path_lens[j] : val_path_lens[j];
        if (n_keys > (size_t)TABLE_MAX_KEYS) {
            ctx_set_error(ctx, "sjhip_group_paths: the paths hold more than %d keys together (found at %s column %u)", TABLE_MAX_KEYS,
                          is_key ? "key" : "value", j);
            return SJHIP_ERR_ARG;
        }
    }
    if (n_keys && (!keys || !key_lens)) {
        ctx_set_error(ctx, "sjhip_group_paths: a null argument (%zu keys are announced)", n_keys);
        return SJHIP_ERR_ARG;
    }
    for (size_t j = 0; j < n_keys; j++) bytes += key_lens[j];
    if (bytes > (size_t)TABLE_MAX_BYTES) {
        ctx_set_error(ctx, "sjhip_group_paths: the keys of the paths are longer than %d bytes together", TABLE_MAX_BYTES);
        return SJHIP_ERR_ARG;
    }
    std::vector<WholePath> k(n_paths);
    size_t key_at = 0, byte_at = 0;
    for (uint32_t c = 0; c < n_paths; c++) {
        const uint32_t pl = c < n_key_cols ? key_path_lens[c] : val_path_lens[c - n_key_cols];
        k[c].keys = pl ? keys + byte_at : nullptr;
        k[c].key_lens = pl ? key_lens + key_at : nullptr;
        k[c].n_keys = pl;
        for (uint32_t j = 0; j < pl; j++) byte_at += key_lens[key_at + j];
        key_at += pl;
    }
    return group_build(ctx, "sjhip_group_paths", k.data(), key_kinds, key_flags, n_key_cols, val_kinds, n_val_cols, rows, groups, key_bytes);
}
// one key column of kind STRING or INT without a flag -- a row without an OK key is in no group -- and at most one value column
int sjhip_group_path(sjhip_ctx *ctx, const uint8_t *key_keys, const uint32_t *key_key_lens, uint32_t key_n_keys, int key_kind,
                     const uint8_t *val_keys, const uint32_t *val_key_lens, uint32_t val_n_keys, int val_kind, size_t *rows, size_t *groups,
                     size_t *key_bytes) {
    if (!ctx) return SJHIP_ERR_ARG;
    if (!rows || !groups || !key_bytes) {
        ctx_set_error(ctx, "sjhip_group_path: a null size pointer");
        return SJHIP_ERR_ARG;
    }
    if (key_kind != SJHIP_COL_STRING && key_kind != SJHIP_COL_INT) {
        ctx_set_error(ctx, "sjhip_group_path: key kind %d is not SJHIP_COL_STRING or SJHIP_COL_INT", key_kind);
        return SJHIP_ERR_ARG;
    }
    const bool value = val_kind != SJHIP_GROUP_NO_VALUE;
    if (value && val_kind != SJHIP_COL_FLOAT && val_kind != SJHIP_COL_INT && val_kind != SJHIP_COL_UINT) {
        ctx_set_error(ctx, "sjhip_group_path: value kind %d is not SJHIP_COL_FLOAT, SJHIP_COL_INT, SJHIP_COL_UINT or SJHIP_GROUP_NO_VALUE", val_kind);
        return SJHIP_ERR_ARG;
    }
    WholePath kv[2] = {{key_keys, key_key_lens, key_n_keys}, {val_keys, val_key_lens, val_n_keys}};
    return group_build(ctx, "sjhip_group_path", kv, &key_kind, nullptr, 1, &val_kind, value ? 1u : 0u, rows, groups, key_bytes);
}

static int no_grouping(sjhip_ctx *ctx, const char *call) {
    ctx_set_error(ctx, "no grouping on the device (%s follows sjhip_group_path or sjhip_group_paths, with no parse in between)", call);
    return SJHIP_ERR_ARG;
}
static GroupArrays group_arrays(const sjhip_ctx *ctx, const ResultState::Groups &z) {  // the grouping in force
    GroupArrays a;
    (void)group_layout(Carve(ctx->d_group.p), z, &a);
    return a;
}
// Column `col` of a grouping: where its entries lie (its bytes: z.col_bytes[col])
struct GroupColumn {
    const u64 *key_off;  // STRING
    const void *keys;
    const u8 *key_ok, *status;
};
static GroupColumn group_column(const GroupArrays &a, const ResultState::Groups &z, uint32_t col) {
    const int kind = z.key_kinds[col];
    const void *const keys = kind == SJHIP_COL_STRING ? (const void *)a.key_bytes[col]
                                                      : (kind == SJHIP_COL_BOOL ? (const void *)a.key_u8[col] : (const void *)a.key_val[col]);
    return {a.key_off[col], keys, a.key_ok[col], a.status[col]};
}
static int fetch_aggregates(sjhip_ctx *ctx, const ResultState::Groups &z, uint32_t val, void *const (&dst)[6]) {
    if (z.groups == 0) return SJHIP_OK;
    const u64 *const agg = group_arrays(ctx, z).agg[val];
    FetchCopy copies[6];
    for (int j = 0; j < 6; j++) copies[j] = {dst[j], agg + (size_t)j * z.groups, z.groups * 8};
    return fetch_copies(ctx, copies, 6, "D2H group aggregates", "group aggregates fetch sync");
}
int sjhip_fetch_groups(sjhip_ctx *ctx, uint64_t *key_offsets, void *keys, uint64_t *first_row, uint64_t *group_rows, uint32_t *codes,
                       uint8_t *status) {
    if (!ctx) return SJHIP_ERR_ARG;
    if (!ctx->res.groups.exists()) return no_grouping(ctx, "sjhip_fetch_groups");
    const ResultState::Groups &z = ctx->res.groups.sizes();
    if (z.key_cols > 1 && (key_offsets || keys || status)) {
        ctx_set_error(ctx, "sjhip_fetch_groups: the grouping has %u key columns (pass NULL for key_offsets, keys and status; the columns are "
                           "sjhip_fetch_group_keys)", z.key_cols);
        return SJHIP_ERR_ARG;
    }
    const bool strings = z.key_kinds[0] == SJHIP_COL_STRING;
    if (key_offsets && strings && z.groups == 0) key_offsets[0] = 0;
    if (z.rows == 0) return SJHIP_OK;  // (nothing was launched, no arena was written)
    const GroupArrays a = group_arrays(ctx, z);
    const GroupColumn k = group_column(a, z, 0);
    const FetchCopy copies[] = {{strings ? key_offsets : nullptr, k.key_off, (z.groups + 1) * 8}, {keys, k.keys, z.col_bytes[0]},
                                {first_row, a.first_row, z.groups * 8},  {group_rows, a.group_rows, z.groups * 8},
                                {codes, a.codes, z.rows * 4},            {status, k.status, z.rows}};
    return fetch_copies(ctx, copies, 6, "D2H groups", "group fetch sync");
}
int sjhip_fetch_group_keys(sjhip_ctx *ctx, uint32_t col, uint64_t *key_offsets, void *keys, uint8_t *key_ok, uint8_t *status) {
    if (!ctx) return SJHIP_ERR_ARG;
    if (!ctx->res.groups.exists()) return no_grouping(ctx, "sjhip_fetch_group_keys");
    const ResultState::Groups &z = ctx->res.groups.sizes();
    if (col >= z.key_cols) {
        ctx_set_error(ctx, "sjhip_fetch_group_keys: key column %u of a grouping with %u", col, z.key_cols);
        return SJHIP_ERR_ARG;
    }
    const bool strings = z.key_kinds[col] == SJHIP_COL_STRING;
    if (key_offsets && strings && z.groups == 0) key_offsets[0] = 0;
    if (z.rows == 0) return SJHIP_OK;  // (nothing was launched, no arena was written)
    const GroupColumn k = group_column(group_arrays(ctx, z), z, col);
    const FetchCopy copies[] = {{strings ? key_offsets : nullptr, k.key_off, (z.groups + 1) * 8}, {keys, k.keys, z.col_bytes[col]},
                                {key_ok, k.key_ok, z.groups}, {status, k.status, z.rows}};
    return fetch_copies(ctx, copies, 4, "D2H group keys", "group keys fetch sync");
}
int sjhip_fetch_group_aggregates(sjhip_ctx *ctx, uint64_t *count, uint64_t *not_ok, void *sum, uint64_t *sum_hi, void *min, void *max) {
    if (!ctx) return SJHIP_ERR_ARG;
    if (!ctx->res.groups.exists()) return no_grouping(ctx, "sjhip_fetch_group_aggregates");
    const ResultState::Groups &z = ctx->res.groups.sizes();
    if (z.val_cols == 0) {
        ctx_set_error(ctx, "sjhip_fetch_group_aggregates: the grouping has no value column (sjhip_group_path was called with SJHIP_GROUP_NO_VALUE, "
                           "or sjhip_group_paths without value columns)");
        return SJHIP_ERR_ARG;
    }
    if (z.val_cols > 1) {
        ctx_set_error(ctx, "sjhip_fetch_group_aggregates: the grouping has %u value columns (each is sjhip_fetch_group_aggregates_at)", z.val_cols);
        return SJHIP_ERR_ARG;
    }
    return fetch_aggregates(ctx, z, 0, {count, not_ok, sum, sum_hi, min, max});
}
int sjhip_fetch_group_aggregates_at(sjhip_ctx *ctx, uint32_t val, uint64_t *count, uint64_t *not_ok, void *sum, uint64_t *sum_hi, void *min,
                                    void *max) {
    if (!ctx) return SJHIP_ERR_ARG;
    if (!ctx->res.groups.exists()) return no_grouping(ctx, "sjhip_fetch_group_aggregates_at");
    const ResultState::Groups &z = ctx->res.groups.sizes();
    if (val >= z.val_cols) {
        ctx_set_error(ctx, "sjhip_fetch_group_aggregates_at: value column %u of a grouping with %u", val, z.val_cols);
        return SJHIP_ERR_ARG;
    }
    return fetch_aggregates(ctx, z, val, {count, not_ok, sum, sum_hi, min, max});
}

// ---- row schema ----------------------------------------------------------------------------------------------------------------------
// sjhip_row_schema works on the whole result of one context, like the grouping (a sharded one is refused: the dictionaries would
// have to be joined), and reads the selection in force without replacing it.  Two halves with a host round trip each: the member
// walk's count pass on the work arrays of the unnest in d_kat, with the parents' statuses counted beside it -> the members; then,
// in d_schema_work, laid out for that many members, the walk's write pass, the keys, the dictionary and the scans -> the names
// and their bytes; then the product in d_schema (schema_layout), the emit, the sort and the counts, and one wait at the end.
struct SchemaWork {
    unsigned long long *totals;  // [0] names, [1] the bytes of the dictionary
    QSchema s;
    SortWork<u32> sort;
};
static size_t schema_work_layout(Carve c, uint32_t m, SchemaWork *w) {
    const u64 cap = group_table_capacity(m);
    const u32 tiles = tiles_of(m);
    QSchema &s = w->s;
    w->totals = c.take<unsigned long long>(32);
    s.n = m, s.mask = (u32)(cap - 1);
    u64 *const idx = c.take<u64>(m), *const parent = c.take<u64>(m), *const hash = c.take<u64>(m);
    u8 *const cls = c.take<u8>(m);
    u32 *const slot = c.take<u32>(m), *const table = c.take<u32>(cap), *const flag = c.take<u32>((size_t)m + 1);
    u64 *const len = c.take<u64>((size_t)m + 1);
    s.idx = SJ_ARR(idx, m, A_SCHEMA_MEMBER);
    s.parent = SJ_ARR(parent, m, A_SCHEMA_PARENT);
    s.hash = SJ_ARR(hash, m, A_SCHEMA_WORK);
    s.cls = SJ_ARR(cls, m, A_SCHEMA_WORK);
    s.slot = SJ_ARR(slot, m, A_SCHEMA_WORK);
    s.table = SJ_ARR(table, cap, A_SCHEMA_TABLE);
    s.flag = SJ_ARR(flag, (size_t)m + 1, A_SCHEMA_WORK);
    s.len = SJ_ARR(len, (size_t)m + 1, A_SCHEMA_WORK);
    s.tiles_f = c.take<unsigned long long>(tiles);
    s.tiles_l = c.take<unsigned long long>(tiles);
    sort_carve(c, m, &w->sort);
    return c.used;
}
// The schema in d_schema: what the fetch returns, and behind it the run bounds on their way into the counts.
struct SchemaArrays { u64 *name_off, *first_row, *counts, *lo; u8 *name_data; };
static size_t schema_layout(Carve c, const ResultState::Schema &z, SchemaArrays *o) {
    o->name_off = c.take<u64>(z.names + 1);
    o->first_row = c.take<u64>(z.names);
    o->counts = c.take<u64>(z.names * SJHIP_SCHEMA_TYPES);
    o->name_data = c.take<u8>(z.name_bytes);
    o->lo = c.take<u64>(z.names * SJHIP_SCHEMA_TYPES);  // (not part of what is fetched)
    return c.used;
}
// the insert of the product; SJ_EXP builds only (A/B timing; the results stay correct): SJHIP_SCHEMA_ELECT=E picks the
// instantiation with E election rounds among 0 (none: every lane probes for itself), 1, 2, 4, 8, 24
typedef void (*SchemaInsert)(QView, QSchema);
static SchemaInsert schema_insert_kernel() {
#if defined(SJ_EXP)
    const char *e = getenv("SJHIP_SCHEMA_ELECT");
    switch (e ? strtoul(e, nullptr, 0) : (unsigned long)SCHEMA_ELECT_ROUNDS) {
        case 0: return k_q_schema_insert<0>;
        case 1: return k_q_schema_insert<1>;
        case 2: return k_q_schema_insert<2>;
        case 4: return k_q_schema_insert<4>;
        case 8: return k_q_schema_insert<8>;
        case 24: return k_q_schema_insert<24>;
    }
#endif
    return k_q_schema_insert<SCHEMA_ELECT_ROUNDS>;
}
static int schema_build(sjhip_ctx *ctx, const WholePath &k, uint32_t n, size_t *rows, uint64_t *status, uint64_t *members, size_t *names,
                        size_t *name_bytes) {
    const u32 depth = (selected(ctx, true) ? ctx->res.rows.sizes().depth : 0u) + k.pth.n + 1u;  // of the members' values
    ResultState::Schema z;
    z.rows = n;
    *rows = n, *members = 0, *names = *name_bytes = 0;
    for (int s = 0; s <= SJHIP_COL_RANGE; s++) status[s] = 0;
    HIPCHK(hipSetDevice(ctx->device), "hipSetDevice");
    if (n == 0) {
        ctx->res.publish_schema(z);
        return published(ctx, ctx->res.schema.exists());
    }
    hipStream_t st = ctx->stream;
    const dim3 b256(256), one(1), wide(1024);
    unsigned long long *const none = nullptr;
    // ---- the first half: the members counted, the parents' statuses counted ----
    UnnestWork uw;
    unsigned long long *hist = nullptr;
    int rc = reserve_layout(ctx, ctx->d_kat, [&](Carve c) {
        c.used = unnest_layout(c, ctx, n, depth, &uw);
        hist = c.take<unsigned long long>(32);
        return c.used;
    });
    if (rc) return rc;
    rc = unnest_count_enqueue(ctx, ctx, k.q, n, k.pth, true, uw);
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(hist, 0, 256, st), "schema status memset");
    hipLaunchKernelGGL(k_q_schema_status, dim3((n + 256u * SCHEMA_STATUS_STEPS - 1) / (256u * SCHEMA_STATUS_STEPS)), b256, 0, st, uw.u, n,
                       SJ_ARR(hist, 32, A_SCHEMA_HIST));
    HIPCHK(hipGetLastError(), "schema status launch");
    unsigned long long *const h = (unsigned long long *)(ctx->h_scratch + 512);
    HIPCHK(hipMemcpyAsync(h, uw.totals + 1, 8, hipMemcpyDeviceToHost, st), "D2H member count");
    HIPCHK(hipMemcpyAsync(h + 1, hist, 8 * (SJHIP_COL_RANGE + 1), hipMemcpyDeviceToHost, st), "D2H schema statuses");
    HIPCHK(hipStreamSynchronize(st), "schema sync");
    rc = query_bounds_check(ctx);
    if (rc) return rc;
    const u64 m64 = h[0] / 2;  // (the starts: a key and a value for every member)
    for (int s = 0; s <= SJHIP_COL_RANGE; s++) status[s] = h[1 + s];
    if (m64 > (1ull << 28)) {
        ctx_set_error(ctx, "sjhip_row_schema: %llu members (at most 2^28)", (unsigned long long)m64);
        return SJHIP_ERR_TOOBIG;
    }
    const u32 m = (u32)m64;
    z.members = m;
    *members = m;
    if (m == 0) {
        ctx->res.publish_schema(z);
        return published(ctx, ctx->res.schema.exists());
    }
    // ---- the second half: the members, their keys, the dictionary, the names numbered ----
    SchemaWork w;
    rc = reserve_layout(ctx, ctx->d_schema_work, [&](Carve c) { return schema_work_layout(c, m, &w); });
    if (rc) return rc;
    const dim3 per_member((m + 255) / 256), per_entry((m + 1u + 255) / 256);
    const u32 tiles = tiles_of(m);
    unnest_write_enqueue(ctx, k.q, true, uw, w.s.idx, w.s.parent);
    HIPCHK(hipMemsetAsync(w.totals, 0, 256, st), "schema totals memset");
    HIPCHK(hipMemsetAsync(arr_raw(w.s.table), 0xff, ((size_t)w.s.mask + 1) * 4, st), "schema table memset");
    hipLaunchKernelGGL(k_q_schema_keys, per_member, b256, 0, st, k.q, w.s);
    hipLaunchKernelGGL(schema_insert_kernel(), per_member, b256, 0, st, k.q, w.s);
    hipLaunchKernelGGL(k_q_schema_first, per_entry, b256, 0, st, k.q, w.s);
    hipLaunchKernelGGL(k_q_schema_tile_sums, dim3(tiles), dim3(QT), 0, st, w.s, m + 1u);
    hipLaunchKernelGGL(k_tw_scan_sums, one, wide, 0, st, w.s.tiles_f, w.s.tiles_l, none, tiles, w.totals);
    hipLaunchKernelGGL(k_q_schema_tile_apply, dim3(tiles), dim3(QT), 0, st, w.s, m + 1u);
    HIPCHK(hipGetLastError(), "schema launch");
    HIPCHK(hipMemcpyAsync(h, w.totals, 16, hipMemcpyDeviceToHost, st), "D2H schema totals");
    HIPCHK(hipStreamSynchronize(st), "schema dictionary sync");
    rc = query_bounds_check(ctx);
    if (rc) return rc;
    const u32 N = (u32)h[0], keys_n = N * (u32)SJHIP_SCHEMA_TYPES;
    z.names = N, z.name_bytes = (size_t)h[1];
    // ---- the product: the dictionary, the first rows, the counts ----
    SchemaArrays a;
    rc = reserve_layout(ctx, ctx->d_schema, [&](Carve c) { return schema_layout(c, z, &a); });
    if (rc) return rc;
    SchemaOut o;
    o.name_off = SJ_ARR(a.name_off, (size_t)N + 1, A_SCHEMA_OUT);
    o.first_row = SJ_ARR(a.first_row, N, A_SCHEMA_OUT);
    o.name_data = SJ_ARR(a.name_data, z.name_bytes, A_SCHEMA_NAMES);
    HIPCHK(hipMemsetAsync(a.counts, 0, (size_t)keys_n * 8, st), "schema counts memset");
    HIPCHK(hipMemsetAsync(a.lo, 0, (size_t)keys_n * 8, st), "schema bounds memset");
    u32 *const first_keys = w.sort.keys[0];
    hipLaunchKernelGGL(k_q_schema_emit, per_member, b256, 0, st, k.q, w.s, o, N, SJ_ARR(first_keys, m, A_SORT));
    const int at = sort_enqueue(st, m, m, group_pass_mask((u64)keys_n - 1u), false, w.sort);
    const u32 *const skeys = w.sort.keys[at];
    hipLaunchKernelGGL(k_q_schema_bounds, per_member, b256, 0, st, SJ_ARR(skeys, m, A_SORT), m, SJ_ARR(a.lo, keys_n, A_SCHEMA_BOUNDS),
                       SJ_ARR(a.counts, keys_n, A_SCHEMA_OUT));
    hipLaunchKernelGGL(k_q_schema_counts, dim3((keys_n + 255) / 256), b256, 0, st, SJ_ARR((const u64 *)a.lo, keys_n, A_SCHEMA_BOUNDS), keys_n,
                       SJ_ARR(a.counts, keys_n, A_SCHEMA_OUT));
    HIPCHK(hipGetLastError(), "schema emit launch");
    HIPCHK(hipStreamSynchronize(st), "schema build sync");
    rc = query_bounds_check(ctx);
    if (rc) return rc;
    *names = z.names, *name_bytes = z.name_bytes;
    ctx->res.publish_schema(z);
    return published(ctx, ctx->res.schema.exists());
}
int sjhip_row_schema(sjhip_ctx *ctx, const uint8_t *keys, const uint32_t *key_lens, uint32_t n_keys, size_t *rows, uint64_t status[6],
                     uint64_t *members, size_t *names, size_t *name_bytes) {
    if (!ctx) return SJHIP_ERR_ARG;
    if (!rows || !status || !members || !names || !name_bytes) {
        ctx_set_error(ctx, "sjhip_row_schema: a null size pointer");
        return SJHIP_ERR_ARG;
    }
    WholePath k = {keys, key_lens, n_keys};
    uint32_t n = 0;
    const int rc = whole_entry(ctx, "sjhip_row_schema", "the dictionaries of shards are not joined", &k, 1, &n);
    if (rc) return rc;
    // ---- nothing was touched up to here; from here on the last schema is gone (the selection and every other product stay) ----
    ctx->res.drop_schema();
    return schema_build(ctx, k, n, rows, status, members, names, name_bytes);
}
int sjhip_fetch_row_schema(sjhip_ctx *ctx, uint64_t *name_offsets, uint8_t *name_data, uint64_t *first_row, uint64_t *counts) {
    if (!ctx) return SJHIP_ERR_ARG;
    if (!ctx->res.schema.exists())
        return no_product(ctx, "no row schema on the device (sjhip_fetch_row_schema follows sjhip_row_schema, with no parse in between)");
    const ResultState::Schema &z = ctx->res.schema.sizes();
    if (z.names == 0) {  // (nothing was launched for the product, no arena was written)
        if (name_offsets) name_offsets[0] = 0;
        return SJHIP_OK;
    }
    SchemaArrays a;
    (void)schema_layout(Carve(ctx->d_schema.p), z, &a);
    const FetchCopy copies[] = {{name_offsets, a.name_off, (z.names + 1) * 8}, {name_data, a.name_data, z.name_bytes},
                                {first_row, a.first_row, z.names * 8}, {counts, a.counts, z.names * SJHIP_SCHEMA_TYPES * 8}};
    return fetch_copies(ctx, copies, 4, "D2H row schema", "row schema fetch sync");
}

// ---- order ---------------------------------------------------------------------------------------------------------------------------
// sjhip_order_path, sjhip_order_path_strings and sjhip_order_paths work on the whole result of one context (a sharded one is refused:
// the ranks of shards would have to be merged) and differ in their argument checks, in the columns they hand to order_build and in
// the kind of the product.  The work arrays of all kernels (OrderWork) lie in d_kat, laid out once for the row count -- every round
// works on a prefix of them --, the arrays of the narrowing (where_layout) behind them; the product (OrderOut) lies in d_order,
// reserved when the narrowing is through.  One host round trip per round -- the active count and the ANDs / ORs that plan the
// round's two sorts; a string column's first also brings its longest key, which bounds its rounds --, the wait of the narrowing,
// one wait at the end.
struct OrderCol {
    QView q;  // (the keys of the column's path are the view's)
    QPath pth;
    int kind;
    u32 desc;
};
struct OrderWork {
    QOrder o;
    u8 *status0, *status_c;  // [n] each: column 0's statuses, and those of the column at work behind it
    SortWork<u64> sort;      // by chunk key
    SortWork<u32> csort;     // by class key
    QWhere w;
    WhereNew nw;
    unsigned long long *w_totals;
};
static size_t order_work_layout(Carve c, const sjhip_ctx *ctx, uint32_t n, OrderWork *w) {
    const u32 tiles = (n + QTILE - 1) / QTILE;
    QOrder &o = w->o;
    o.totals = c.take<unsigned long long>(32);
    o.n = n;
    w->status0 = c.take<u8>(n), w->status_c = c.take<u8>(n);
    u8 *const flags = c.take<u8>(n), *const bnd = c.take<u8>((size_t)n + 1);
    u64 *const kidx = c.take<u64>(n), *const chunk = c.take<u64>(n);
    u32 *const perm = c.take<u32>(n), *const ckey = c.take<u32>(n);
    u32 *const row = c.take<u32>(n), *const pos = c.take<u32>(n), *const cls = c.take<u32>(n);
    u32 *const row_out = c.take<u32>(n), *const pos_out = c.take<u32>(n), *const cls_out = c.take<u32>(n);
    o.status = SJ_ARR(w->status0, n, A_ORDER_ROW);
    o.kidx = SJ_ARR(kidx, n, A_ORDER_ROW);
    o.perm = SJ_ARR(perm, n, A_SORT);
    o.flags = SJ_ARR(flags, n, A_ORDER_ACT);
    o.chunk = SJ_ARR(chunk, n, A_ORDER_ACT);
    o.ckey = SJ_ARR(ckey, n, A_ORDER_ACT);
    o.row = SJ_ARR(row, n, A_ORDER_ACT), o.pos = SJ_ARR(pos, n, A_ORDER_ACT), o.cls = SJ_ARR(cls, n, A_ORDER_ACT);
    o.row_out = SJ_ARR(row_out, n, A_ORDER_ACT), o.pos_out = SJ_ARR(pos_out, n, A_ORDER_ACT), o.cls_out = SJ_ARR(cls_out, n, A_ORDER_ACT);
    o.bnd = SJ_ARR(bnd, (size_t)n + 1, A_ORDER_BND);
    unsigned long long **const per_tile[] = {&o.tiles_ok, &o.tiles_len, &o.tiles_kand, &o.tiles_kor, &o.tiles_cand, &o.tiles_cor, &o.tiles_head, &o.tiles_act};
    for (unsigned long long **t : per_tile) *t = c.take<unsigned long long>(tiles);
    sort_carve(c, n, &w->sort);
    sort_carve(c, n, &w->csort);
    (void)(c.used = where_layout(c, ctx, n, &w->w, &w->nw, &w->w_totals));
    return c.used;
}
// The order in d_order: what the fetch returns, and nothing else.
struct OrderArrays {
    u64 *order, *values;
    u8 *status;
};
// (kind SJHIP_COL_STRING -- sjhip_order_path_strings -- and ORDER_KIND_MULTI -- sjhip_order_paths -- have no values)
static size_t order_layout(Carve c, size_t rows, int kind, OrderArrays *o) {
    o->order = c.take<u64>(rows);
    o->values = kind == SJHIP_COL_STRING || kind == ORDER_KIND_MULTI ? nullptr : c.take<u64>(rows);
    o->status = c.take<u8>(rows);
    return c.used;
}
// behind the checks of the order call `fn`: cols[c].q is the view of the n > 0 rows in force; kind: the product's -- that of the
// one numeric column of sjhip_order_path, whose values are emitted, SJHIP_COL_STRING or ORDER_KIND_MULTI
static int order_build(sjhip_ctx *ctx, const char *fn, const OrderCol *cols, uint32_t n_cols, int kind, const uint8_t *keys, size_t klen,
                       uint32_t n, uint64_t limit, size_t *records, size_t *rows) {
    OrderWork w;
    int rc = reserve_layout(ctx, ctx->d_kat, [&](Carve c) { return order_work_layout(c, ctx, n, &w); });
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    const u32 tiles = (n + QTILE - 1) / QTILE;
    const dim3 per_row((n + 255) / 256), per_tile(tiles), b256(256), bqt(QT), one(1), wide(1024);
    unsigned long long *const none = nullptr;
    QOrder &o = w.o;
    u64 *const keys0 = w.sort.keys[0];
    u32 *const rows0 = w.sort.rows[0], *const ckeys0 = w.csort.keys[0], *const crows0 = w.csort.rows[0];
    const unsigned long long *const active = o.totals + ORDER_T_ACTIVE;
    // a single-key call parks the rows without a key in front of its rounds (k_q_order_park), and a numeric key needs no rounds:
    // one sort of the OK rows orders it
    const bool single = n_cols == 1, direct = single && cols[0].kind != SJHIP_COL_STRING;
    const u32 *ranked = arr_raw(o.perm);
    HIPCHK(hipMemsetAsync(o.totals, 0, 256, st), "order totals memset");
    if (!single) hipLaunchKernelGGL(k_q_order_init, per_row, b256, 0, st, o);
    unsigned long long *const h = (unsigned long long *)(ctx->h_scratch + 512), *const h_left = (unsigned long long *)(ctx->h_scratch + 1024);
    for (uint32_t c = 0; c < n_cols; c++) h_left[c] = 0;
    u64 left_bound[ORDER_MAX_KEYS] = {};
    bool tied = true;  // rows still tie: the next column has work
    for (uint32_t c = 0; c < n_cols && tied; c++) {
        const OrderCol &col = cols[c];
        const bool is_string = col.kind == SJHIP_COL_STRING;
        if (c > 0) {  // the entries that are not alone in their class, from the boundaries
            hipLaunchKernelGGL(k_q_order_bounds, per_tile, bqt, 0, st, o);
            hipLaunchKernelGGL(k_tw_scan_sums, one, wide, 0, st, o.tiles_head, o.tiles_act, none, tiles, o.totals + ORDER_T_HEADS);
            hipLaunchKernelGGL(k_q_order_rebuild, per_tile, bqt, 0, st, o);
            o.status = SJ_ARR(w.status_c, n, A_ORDER_ROW);
        }
        hipLaunchKernelGGL(k_q_order_keys, per_tile, bqt, 0, st, col.q, col.pth, o, col.kind, col.desc, c == 0 ? 1u : 0u, active);
        if (single) {
            u64 *const pairs = direct ? keys0 : nullptr;
            u32 *const rows1 = w.sort.rows[1];
            hipLaunchKernelGGL(k_tw_scan_sums, one, wide, 0, st, o.tiles_ok, none, none, tiles, o.totals + ORDER_T_ACTIVE);
            hipLaunchKernelGGL(k_q_order_park, per_tile, bqt, 0, st, o, SJ_ARR(pairs, n, A_SORT), SJ_ARR(rows0, n, A_SORT), SJ_ARR(rows1, n, A_SORT));
        }
        if (direct) {  // the pass plan from the AND and the OR of the keys; fewer than two OK rows: no pass
            hipLaunchKernelGGL(k_q_order_fold, one, bqt, 0, st, o, tiles, 0u);
            HIPCHK(hipGetLastError(), "order launch");
            HIPCHK(hipMemcpyAsync(h, o.totals, ORDER_T_WORDS * 8, hipMemcpyDeviceToHost, st), "D2H order totals");
            HIPCHK(hipStreamSynchronize(st), "order sync");
            rc = query_bounds_check(ctx);
            if (rc) return rc;
            const u32 n_ok = (u32)h[ORDER_T_ACTIVE], mask = n_ok > 1 ? order_pass_mask(h[ORDER_T_ANDOR], h[ORDER_T_ANDOR + 1]) : 0u;
            ranked = w.sort.rows[sort_enqueue(st, n_ok, n, mask, true, w.sort)];
            break;
        }
        u64 bound = 1;  // of the column's rounds: a string column's is known after its first copy
        u32 m_max = n;  // the round's active entries are at most this many
        for (u64 round = 0;; round++) {
            // the round's chunk keys, and its one round trip
            const u32 ctiles = (m_max + QTILE - 1) / QTILE;
            hipLaunchKernelGGL(k_q_order_chunks, dim3(ctiles), bqt, 0, st, col.q, o, col.kind, col.desc, active, round * (u64)STRORD_CHUNK,
                               SJ_ARR(keys0, n, A_SORT), SJ_ARR(rows0, n, A_SORT));
            hipLaunchKernelGGL(k_q_order_fold, one, bqt, 0, st, o, ctiles, round == 0 ? tiles : 0u);
            HIPCHK(hipGetLastError(), "order chunk launch");
            HIPCHK(hipMemcpyAsync(h, o.totals, ORDER_T_WORDS * 8, hipMemcpyDeviceToHost, st), "D2H order totals");
            HIPCHK(hipStreamSynchronize(st), "order sync");
            rc = query_bounds_check(ctx);
            if (rc) return rc;
            if (round == 0 && is_string) bound = strord_max_rounds(h[ORDER_T_LONGEST]);
            const u32 m = (u32)h[ORDER_T_ACTIVE];
            if (m < 2) {  // (a class has two members at least: nothing is active)
                tied = round > 0;  // (behind the column's first round the classes it finished may still hold ties)
                break;
            }
            // stable by (class key, chunk key): the chunk keys first -- of the OK rows; without one, no digit --, then the class keys
            const u64 kand = h[ORDER_T_ANDOR], kor = h[ORDER_T_ANDOR + 1];
            const u32 kmask = (kand & ~kor) ? 0u : order_pass_mask(kand, kor);
            const u32 cmask = order_pass_mask(h[ORDER_T_ANDOR + 2], h[ORDER_T_ANDOR + 3]);
            const u32 *sorted = w.sort.rows[sort_enqueue(st, m, n, kmask, true, w.sort)];
            const dim3 per_entry((m + 255) / 256), per_etile((m + QTILE - 1) / QTILE);
            if (cmask) {
                hipLaunchKernelGGL(k_q_order_classes, per_entry, b256, 0, st, o.ckey, m, SJ_ARR(sorted, n, A_SORT), SJ_ARR(ckeys0, n, A_SORT),
                                   SJ_ARR(crows0, n, A_SORT));
                sorted = w.csort.rows[sort_enqueue(st, m, n, cmask, true, w.csort)];
            }
            // place, mark; a string column renumbers and compacts what stays in it
            hipLaunchKernelGGL(k_q_order_place, per_etile, bqt, 0, st, o, m, SJ_ARR(sorted, n, A_SORT), is_string ? 1u : 0u, col.desc);
            if (is_string) {
                hipLaunchKernelGGL(k_tw_scan_sums, one, wide, 0, st, o.tiles_head, o.tiles_act, none, per_etile.x, o.totals + ORDER_T_HEADS);
                hipLaunchKernelGGL(k_q_order_compact, per_etile, bqt, 0, st, o, m, SJ_ARR(sorted, n, A_SORT));
                std::swap(o.row, o.row_out), std::swap(o.pos, o.pos_out), std::swap(o.cls, o.cls_out);
            }
            HIPCHK(hipGetLastError(), "order round launch");
            m_max = m;
            if (round + 1 >= bound) {  // the column's last round: what a string column left active (nothing) is looked at with the emit's wait
                if (is_string) {
                    HIPCHK(hipMemcpyAsync(h_left + c, o.totals + ORDER_T_ACTIVE, 8, hipMemcpyDeviceToHost, st), "D2H order rest");
                    left_bound[c] = bound;
                }
                break;
            }
        }
    }
    // rank, flag, narrow: the first `kept` ranks stay
    const size_t kept = limit == 0 || limit >= n ? (size_t)n : (size_t)limit;
    hipLaunchKernelGGL(k_q_order_flag, per_row, b256, 0, st, SJ_ARR(ranked, n, A_SORT), n, (u64)kept, w.w.flag);
    hipLaunchKernelGGL(k_q_order_flag_sums, per_tile, bqt, 0, st, w.w.flag, n, w.w.tiles);
    hipLaunchKernelGGL(k_tw_scan_sums, one, wide, 0, st, w.w.tiles, none, none, tiles, none);
    HIPCHK(hipGetLastError(), "order flag launch");
    const std::vector<sjhip_ctx *> parts(1, ctx);
    rc = where_narrow(ctx, parts, keys, klen, &NO_VALUE, 0, std::vector<QWhere>(1, w.w), std::vector<WhereNew>(1, w.nw),
                      std::vector<size_t>(1, kept), records, rows);
    if (rc) return rc;
    OrderArrays a;
    rc = reserve_layout(ctx, ctx->d_order, [&](Carve c) { return order_layout(c, kept, kind, &a); });
    if (rc) return rc;
    OrderOut out;
    out.order = SJ_ARR(a.order, kept, A_ORDER_OUT);
    out.values = SJ_ARR(a.values, kept, A_ORDER_OUT);
    out.status = SJ_ARR(a.status, kept, A_ORDER_OUT);
    // (column 0's status: the only column every row is evaluated on.  A product with values has one numeric column: kidx holds its keys)
    const u8 *const status = w.status0;
    const u64 *const values_of = a.values ? arr_raw(o.kidx) : nullptr;
    const u32 *const pre = arr_raw(w.w.pre);
    hipLaunchKernelGGL(k_q_order_emit, dim3(((u32)kept + 255) / 256), b256, 0, st, SJ_ARR(ranked, n, A_SORT), SJ_ARR(status, n, A_ORDER_ROW),
                       SJ_ARR(values_of, n, A_ORDER_ROW), cols[0].kind, cols[0].desc, SJ_ARR(pre, n, A_WHERE_PRE), (u32)kept, out);
    HIPCHK(hipGetLastError(), "order emit launch");
    HIPCHK(hipStreamSynchronize(st), "order emit sync");
    rc = query_bounds_check(ctx);
    if (rc) return rc;
    for (uint32_t c = 0; c < n_cols; c++)
        if (h_left[c]) {
            if (single)
                ctx_set_error(ctx, "%s: %llu rows are still unordered after %llu rounds, the bound of the longest key (%llu bytes)", fn, h_left[c],
                              (unsigned long long)left_bound[c], (unsigned long long)left_bound[c] * STRORD_CHUNK - 1);
            else
                ctx_set_error(ctx, "%s: column %u: %llu rows are still unordered after %llu rounds, the bound of its longest key", fn, c, h_left[c],
                              (unsigned long long)left_bound[c]);
            return SJHIP_ERR_HIP;
        }
    return published(ctx, ctx->res.publish(&ResultState::order, {kept, kind}));
}

// two argument checks of the order call `fn`, made where each call made them: the size pointers; the flags of a column (col < 0: of
// the call's only one)
static int order_sizes_check(sjhip_ctx *ctx, const char *fn, const size_t *records, const size_t *rows) {
    if (records && rows) return SJHIP_OK;
    ctx_set_error(ctx, "%s: a null size pointer", fn);
    return SJHIP_ERR_ARG;
}
static int order_flags_check(sjhip_ctx *ctx, const char *fn, int col, uint32_t flags) {
    if (!(flags & ~SJHIP_ORDER_DESC)) return SJHIP_OK;
    if (col < 0) ctx_set_error(ctx, "%s: unknown flag bits 0x%x", fn, flags & ~SJHIP_ORDER_DESC);
    else ctx_set_error(ctx, "%s: column %d: unknown flag bits 0x%x", fn, col, flags & ~SJHIP_ORDER_DESC);
    return SJHIP_ERR_ARG;
}
// behind the argument checks of the order call `fn`: the n_cols paths made and viewed (whole_entry), the last order given up, the
// empty selection, the build (flags null: all ascending)
static int order_entry(sjhip_ctx *ctx, const char *fn, WholePath *k, const int *kinds, const uint32_t *flags, uint32_t n_cols, int kind,
                       uint64_t limit, size_t *records, size_t *rows) {
    uint32_t n = 0;
    int rc = whole_entry(ctx, fn, "the ranks of shards are not merged", k, (int)n_cols, &n);
    if (rc) return rc;
    // ---- nothing was touched up to here; from here on the last order is gone ----
    ctx->res.order.begin();
    HIPCHK(hipSetDevice(ctx->device), "hipSetDevice");
    if (n == 0) {  // (a selection without rows: it stays as it is)
        *records = ctx->res.rows.sizes().records, *rows = 0;
        return published(ctx, ctx->res.publish(&ResultState::order, {0, kind}));
    }
    OrderCol cols[ORDER_MAX_KEYS];
    for (uint32_t c = 0; c < n_cols; c++) cols[c] = {k[c].q, k[c].pth, kinds[c], flags ? flags[c] & SJHIP_ORDER_DESC : 0u};
    rc = order_build(ctx, fn, cols, n_cols, kind, k[0].keys, k[0].klen, n, limit, records, rows);
    if (rc) {  // half-built: the old selection may have been written over
        ctx->res.rows.begin();
        char why[sizeof ctx->err];
        snprintf(why, sizeof why, "%s", ctx->err);
        ctx_set_error(ctx, "%s failed and the row selection was given up: %.170s", fn, why);
    }
    return rc;
}

int sjhip_order_path(sjhip_ctx *ctx, const uint8_t *keys, const uint32_t *key_lens, uint32_t n_keys, int kind, uint32_t flags,
                     uint64_t limit, size_t *records, size_t *rows) {
    if (!ctx) return SJHIP_ERR_ARG;
    if (order_sizes_check(ctx, "sjhip_order_path", records, rows)) return SJHIP_ERR_ARG;
    if (kind != SJHIP_COL_FLOAT && kind != SJHIP_COL_INT && kind != SJHIP_COL_UINT) {
        ctx_set_error(ctx, "sjhip_order_path: key kind %d is not SJHIP_COL_FLOAT, SJHIP_COL_INT or SJHIP_COL_UINT", kind);
        return SJHIP_ERR_ARG;
    }
    if (order_flags_check(ctx, "sjhip_order_path", -1, flags)) return SJHIP_ERR_ARG;
    WholePath k = {keys, key_lens, n_keys};
    return order_entry(ctx, "sjhip_order_path", &k, &kind, &flags, 1, kind, limit, records, rows);
}

int sjhip_order_path_strings(sjhip_ctx *ctx, const uint8_t *keys, const uint32_t *key_lens, uint32_t n_keys, uint32_t flags, uint64_t limit,
                             size_t *records, size_t *rows) {
    if (!ctx) return SJHIP_ERR_ARG;
    if (order_sizes_check(ctx, "sjhip_order_path_strings", records, rows)) return SJHIP_ERR_ARG;
    if (order_flags_check(ctx, "sjhip_order_path_strings", -1, flags)) return SJHIP_ERR_ARG;
    const int kind = SJHIP_COL_STRING;
    WholePath k = {keys, key_lens, n_keys};
    return order_entry(ctx, "sjhip_order_path_strings", &k, &kind, &flags, 1, kind, limit, records, rows);
}

int sjhip_order_paths(sjhip_ctx *ctx, const uint8_t *keys, const uint32_t *key_lens, const uint32_t *path_lens, const int *kinds,
                      const uint32_t *flags, uint32_t n_cols, uint64_t limit, size_t *records, size_t *rows) {
    if (!ctx) return SJHIP_ERR_ARG;
    if (order_sizes_check(ctx, "sjhip_order_paths", records, rows)) return SJHIP_ERR_ARG;
    if (n_cols < 1 || n_cols > (uint32_t)SJHIP_ORDER_MAX_KEYS) {
        ctx_set_error(ctx, "sjhip_order_paths: %u key columns (1 to %d)", n_cols, SJHIP_ORDER_MAX_KEYS);
        return SJHIP_ERR_ARG;
    }
    if (!path_lens || !kinds) {
        ctx_set_error(ctx, "sjhip_order_paths: a null argument (path_lens, kinds)");
        return SJHIP_ERR_ARG;
    }
    size_t n_keys = 0, bytes = 0;
    for (uint32_t c = 0; c < n_cols; c++) {
        const int kind = kinds[c];
        if (kind != SJHIP_COL_FLOAT && kind != SJHIP_COL_INT && kind != SJHIP_COL_UINT && kind != SJHIP_COL_STRING) {
            ctx_set_error(ctx, "sjhip_order_paths: column %u: key kind %d is not SJHIP_COL_FLOAT, SJHIP_COL_INT, SJHIP_COL_UINT or SJHIP_COL_STRING", c,
                          kind);
            return SJHIP_ERR_ARG;
        }
        if (flags && order_flags_check(ctx, "sjhip_order_paths", (int)c, flags[c])) return SJHIP_ERR_ARG;
        n_keys += path_lens[c];
        if (n_keys > (size_t)TABLE_MAX_KEYS) {
            ctx_set_error(ctx, "sjhip_order_paths: the paths hold more than %d keys together (found at column %u)", TABLE_MAX_KEYS, c);
            return SJHIP_ERR_ARG;
        }
    }
    if (n_keys && (!keys || !key_lens)) {
        ctx_set_error(ctx, "sjhip_order_paths: a null argument (%zu keys are announced)", n_keys);
        return SJHIP_ERR_ARG;
    }
    for (size_t j = 0; j < n_keys; j++) bytes += key_lens[j];
    if (bytes > (size_t)TABLE_MAX_BYTES) {
        ctx_set_error(ctx, "sjhip_order_paths: the keys of the paths are longer than %d bytes together", TABLE_MAX_BYTES);
        return SJHIP_ERR_ARG;
    }
    WholePath k[SJHIP_ORDER_MAX_KEYS] = {};
    size_t key_at = 0, byte_at = 0;
    for (uint32_t c = 0; c < n_cols; c++) {
        k[c].keys = path_lens[c] ? keys + byte_at : nullptr;
        k[c].key_lens = path_lens[c] ? key_lens + key_at : nullptr;
        k[c].n_keys = path_lens[c];
        for (uint32_t j = 0; j < path_lens[c]; j++) byte_at += key_lens[key_at + j];
        key_at += path_lens[c];
    }
    return order_entry(ctx, "sjhip_order_paths", k, kinds, flags, n_cols, ORDER_KIND_MULTI, limit, records, rows);
}

int sjhip_fetch_order(sjhip_ctx *ctx, uint64_t *order, void *values, uint8_t *status) {
    if (!ctx) return SJHIP_ERR_ARG;
    if (!ctx->res.order.exists()) {
        ctx_set_error(ctx, "no order on the device (sjhip_fetch_order follows sjhip_order_path, with no parse in between)");
        return SJHIP_ERR_ARG;
    }
    const size_t kept = ctx->res.order.sizes().rows;
    const int kind = ctx->res.order.sizes().kind;
    if (values && kind == SJHIP_COL_STRING) {
        ctx_set_error(ctx, "sjhip_fetch_order: a string order has no 8-byte values (pass NULL; the keys are sjhip_extract_path_strings on the kept "
                           "rows, taken through order[])");
        return SJHIP_ERR_ARG;
    }
    if (values && kind == ORDER_KIND_MULTI) {
        ctx_set_error(ctx, "sjhip_fetch_order: an order by several keys has no 8-byte values (pass NULL; the keys are sjhip_extract_table on the "
                           "kept rows, taken through order[])");
        return SJHIP_ERR_ARG;
    }
    if (kept == 0) return SJHIP_OK;  // (nothing was launched, no arena was written)
    OrderArrays a;
    (void)order_layout(Carve(ctx->d_order.p), kept, kind, &a);
    const FetchCopy copies[] = {{order, a.order, kept * 8}, {values, a.values, kept * 8}, {status, a.status, kept}};
    return fetch_copies(ctx, copies, 3, "D2H order", "order fetch sync");
}
