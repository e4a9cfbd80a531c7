// sj_bounds.h -- bounds-checked views of the device arenas for the debug build (-DSJ_DEBUG_BOUNDS).
//
// The stage-1 kernels write positions, kinds and the string masks through such views as well (stage1.hip).
// The kernels of stage2.hip reach every array of the parse -- message, positions, kinds, the stage-2 work arrays, the
// string masks and records, tape and Strings.B -- through the fields of S2Dev / StrView.  Those fields are declared as
// Arr<T>: in the product build that is a plain T* (no code changes, no cost); in the debug build it is a pointer with
// its element count, every a[i] is checked, and every place that forms a pointer for a wider access (a 16-byte load
// of four positions, a window of the message handed to the number parser) states how many elements it is going to
// touch: arr_at(a, first, count).  A violation is recorded (array id, index, size; the first one wins) and the access
// is redirected to an element inside the array, so the kernel finishes, nothing outside the arena is touched, and the
// host turns the record into an error of the parse (parse_api.hip) -- a test suite run under this build
// (tools/gpu_debug_bounds.sh) fails on the first out-of-bounds access anywhere in the parse path instead of relying on
// the access landing on an unmapped page.  SURVEY.md section 5 (sanitizer / race-detection row).
#pragma once
#include <stdint.h>

#include <type_traits>

#include "sj_chunk.h"  // SJ_HD

namespace sj {

// array ids (reported with a hit)
enum ArrId : uint32_t {
    A_NONE = 0, A_MSG, A_POS, A_KIND, A_DLEN, A_STR_OFF, A_NL_OFF, A_NUMQ, A_BIGQ, A_STRQ, A_BR_DEPTH, A_BR_OFF, A_BR_INFO, A_AGG,
    A_LEV, A_TAPE, A_STRINGS, A_STR_OUT, A_REC, A_UNIT_CNT, A_SV_BASE, A_SV_QM, A_SV_Q, A_SV_ST, A_SV_UNIT_H, A_SV_UNIT_SLOW,
    A_SELFTEST, A_KEYFLAG,
    A_UNIT_COPY, A_S1_POS, A_S1_KIND, A_S1_QM, A_S1_Q, A_S1_ST, A_S1_UNIT_H, A_S1_UNIT_SLOW,  // stage 1's outputs (stage1.hip)
    A_S1_REC, A_S1_UNIT_CNT, A_S1_UNIT_COPY, A_S1_UNIT_STR, A_UNIT_STR, A_SOFF,
    A_S1_TILE_UNIT, A_TILE_UNIT, A_UNIT_TQ,
    A_COL,  // the bytes of a string column (query.hip)
    A_LIST_VAL, A_LIST_SOFF, A_LIST_DATA,  // a list column (query.hip): its values / its string offsets / its string bytes
    // a table (query.hip): the values and statuses of its numeric columns / the work arrays of its string columns / their bytes
    A_TABLE_OUT, A_TABLE_WORK, A_TABLE_DATA,
    A_ROWS,  // the row index of a row selection (query.hip): written by the compaction, read by every query that runs on rows
    // a row predicate (query.hip, sjhip_where_path): the flag of every current row / the kept rows in front of it / the new row offsets
    A_WHERE_FLAG, A_WHERE_PRE, A_WHERE_OFF,
    // the filtered rows (query.hip, sjhip_filter_rows): the output words of every row and their prefix / the Strings.B range of every
    // row (first string, bytes, their prefix) / the new tape / the new Strings.B (these two: sjhip_filter_where's as well)
    A_FROWS_WORDS, A_FROWS_STR, A_FROWS_TAPE, A_FROWS_STRINGS,
    // the marshaled rows (marshal.hip, sjhip_marshal_rows): the text bytes of every row and their prefix / the row offsets behind the
    // text / the text / the key flags recovered without SJHIP_FLAG_KEY_FLAGS, by tape index
    A_MROWS_OFF, A_MROWS_OUT_OFF, A_MROWS_TEXT, A_MROWS_KF,
    // the aggregates (query.hip, sjhip_aggregate_path): the head flag of every row / the items a level of the segmented reduction
    // hands to the next / the per-record results
    A_AGG_HEAD, A_AGG_ITEMS, A_AGG_OUT,
    // the grouping (query.hip, sjhip_group_path and sjhip_group_paths): the per-row work arrays, column-major where they are per key
    // column (status, key element or value; tuple hash, in-a-group byte, slot, first-row flag) / the key lengths of the STRING
    // columns / the table of row numbers / the group offsets / the per-group and per-row arrays of the product / the bytes of a
    // STRING column's entries
    A_GROUP_ROW, A_GROUP_LEN, A_GROUP_TABLE, A_GROUP_OFF, A_GROUP_OUT, A_GROUP_KEYS,
    // the ordering (query.hip, sjhip_order_path, _strings and sjhip_order_paths): the per-row work arrays (the statuses on column 0
    // and on the column at work, the key or key element) / the arrays of the active entries (row, position, class, chunk key, class
    // key, head and active flags) / the boundary bytes of the n + 1 positions / the arrays of the product (order, values, status).
    // Its ranked rows and its sorts are A_SORT
    A_ORDER_ROW, A_ORDER_ACT, A_ORDER_BND, A_ORDER_OUT,
    // the radix sort of both (sj_sort.h): the keys and rows of its buffers, and the sorted rows wherever they are read / its digit
    // histograms
    A_SORT, A_SORT_HIST,
    // the unnested rows (query.hip, sjhip_unnest_rows): the target range of every parent row / the status byte of every parent, in
    // the work arrays and in the product / the parent number of every new row / the parent offsets.  The member rows
    // (sjhip_unnest_members) run on the same arrays under the same ids; their names are read through A_TAPE and written through
    // A_COL (sjhip_extract_row_names), their predicate marks through A_WHERE_* (sjhip_where_row_names)
    A_UNNEST_RANGE, A_UNNEST_STATUS, A_UNNEST_PARENT, A_UNNEST_OFF,
    // the packing kernel of the batch (batch_api.hip, k_batch_pack): the caller's device buffer up to the end of its last document /
    // the document descriptors / the packed message
    A_BATCH_SRC, A_BATCH_DOCS, A_BATCH_DST,
    // the projected rows (marshal.hip, sjhip_marshal_rows_paths): the tape index or path status of every cell, column-major / the
    // text bytes of every row and their prefix / the name pieces / where each begins (text and row offsets: A_MROWS_TEXT, _OUT_OFF)
    A_MPROJ_IDX, A_MPROJ_OFF, A_MPROJ_NAMES, A_MPROJ_NAME_OFF,
    // the row schema (query.hip, sjhip_row_schema): the value index of every member (written by the member walk) / its parent row /
    // the per-member work arrays (hash, type class, slot, first-occurrence flag, name length) / the table of member numbers / the
    // status histogram / the run bounds of the sorted (name, type) keys / the arrays of the product (name offsets, first rows,
    // counts) / the names' bytes.  Its sort is A_SORT
    A_SCHEMA_MEMBER, A_SCHEMA_PARENT, A_SCHEMA_WORK, A_SCHEMA_TABLE, A_SCHEMA_HIST, A_SCHEMA_BOUNDS, A_SCHEMA_OUT, A_SCHEMA_NAMES,
    // the set of a set predicate (query.hip, sjhip_where_path_in; sj_wherein.h): the values or the offsets of the string values /
    // the string values' bytes / the hash of every value / the table of value indices
    A_IN_VALS, A_IN_BYTES, A_IN_HASH, A_IN_TABLE
};

#if defined(SJ_DEBUG_BOUNDS)

struct BoundsHit {
    unsigned int hits, id;
    unsigned long long index, size;
};
#if defined(__HIPCC__)
static __device__ BoundsHit g_bounds_hit;                 // one per translation unit; each reads and clears its own (bounds_take)
static __device__ unsigned long long g_bounds_sink[8];    // target of accesses to an array without a single element
__device__ __forceinline__ void bounds_report(uint32_t id, unsigned long long index, unsigned long long size) {
    if (atomicAdd(&g_bounds_hit.hits, 1u) == 0u) {
        g_bounds_hit.id = id;
        g_bounds_hit.index = index;
        g_bounds_hit.size = size;
    }
}
// host: this translation unit's record, read and cleared (false, and an empty record: it could not be read)
static inline bool bounds_take(BoundsHit *h) {
    *h = BoundsHit{};
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_bounds_hit), sizeof *h) != hipSuccess) return false;
    if (h->hits) {
        const BoundsHit zero = {};
        (void)hipMemcpyToSymbol(HIP_SYMBOL(g_bounds_hit), &zero, sizeof zero);
    }
    return true;
}
#else
inline void bounds_report(uint32_t, unsigned long long, unsigned long long) {}
static unsigned long long g_bounds_sink[8];
#endif

template <typename T>
struct Arr {
    T *p = nullptr;
    unsigned long long n = 0;  // elements
    uint32_t id = A_NONE;
    Arr() = default;
    SJ_HD Arr(T *p_, unsigned long long n_, uint32_t id_) : p(p_), n(n_), id(id_) {}
    SJ_HD Arr(decltype(nullptr)) {}
    template <typename U>
    SJ_HD Arr(const Arr<U> &o) : p(o.p), n(o.n), id(o.id) {}  // Arr<T> -> Arr<const T>
    SJ_HD explicit operator bool() const { return p != nullptr; }
    SJ_HD bool operator!() const { return p == nullptr; }
    SJ_HD T &operator[](unsigned long long i) const {
        if (i >= n) {
            bounds_report(id, i, n);
            if (n == 0) return *reinterpret_cast<T *>(g_bounds_sink);
            i = n - 1;
        }
        return p[i];
    }
    // pointer to elements [first, first + count)
    SJ_HD T *at(unsigned long long first, unsigned long long count) const {
        if (first > n || count > n - first) {
            bounds_report(id, first + count, n);
            if (count > n) return reinterpret_cast<T *>(g_bounds_sink);
            first = n - count;
        }
        return p + first;
    }
};
template <typename T>
SJ_HD T *arr_at(const Arr<T> &a, unsigned long long first, unsigned long long count) { return a.at(first, count); }
template <typename T>
SJ_HD T *arr_raw(const Arr<T> &a) { return a.p; }  // (launchers: memsets and copies of whole arrays)
#define SJ_ARR(ptr, count, id) ::sj::Arr<typename std::remove_pointer<decltype(ptr)>::type>((ptr), (unsigned long long)(count), (id))
#define SJ_ARR_PARAM(T) ::sj::Arr<T>  // a function parameter that is `T *__restrict__` in the product build

#else  // product build: plain pointers

template <typename T>
using Arr = T *;
template <typename T>
SJ_HD T *arr_at(T *a, unsigned long long first, unsigned long long) { return a + first; }
template <typename T>
SJ_HD T *arr_raw(T *a) { return a; }
#define SJ_ARR(ptr, count, id) (ptr)
#define SJ_ARR_PARAM(T) T *__restrict__

#endif

}  // namespace sj

// ---- streaming stores ------------------------------------------------------------------------------------------------
// Output that nobody reads again soon (stage 1's positions, the tape, Strings.B) leaves with the nt bit: it does not displace the
// lines the following kernels -- or the next pass over the same message -- find in the L2 / Infinity Cache (round 6, measured).
#if defined(__HIPCC__)
namespace sj {
template <typename T>
__device__ __forceinline__ void nt_store(T *p, T v) { __builtin_nontemporal_store(v, p); }
__device__ __forceinline__ void nt_store4(void *p, uint4 v) {  // (merged into one global_store_dwordx4 ... nt)
    unsigned int *d = reinterpret_cast<unsigned int *>(p);
    __builtin_nontemporal_store(v.x, d);
    __builtin_nontemporal_store(v.y, d + 1);
    __builtin_nontemporal_store(v.z, d + 2);
    __builtin_nontemporal_store(v.w, d + 3);
}
}  // namespace sj
#endif

