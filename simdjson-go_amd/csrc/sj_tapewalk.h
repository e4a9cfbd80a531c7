// sj_tapewalk.h -- device helpers shared by the kernels that walk a finished tape (serialize.hip, marshal.hip, query.hip):
// 2048-word tiles, block-wide scans, the one-block scans over per-tile values, and the tag / raw-word classification.
//
// A tape entry is one word (brackets, roots, atoms) or two (strings: tag + length, numbers: tag + value).  The second
// word is raw 64-bit data whose top byte can look like any tag, so "is this word a tag?" is not a local question.
// Raw words only ever follow a two-word tag (" l u d) that is itself not raw; with c(i) = "the top byte of word i is
// one of \" l u d" and p = the last index below i with c(p) = 0 (an anchor; word 0, the opening root, is one):
//     word i is raw  <=>  i - p - 1 is odd.
// k_tw_last / k_tw_scan_last give every tile the last anchor in front of it; inside a tile a block max-scan does it.
// The kernels that walk one row or record per wave apply the rule through tw_walk_span -- the one place that spells it for 64
// words per step -- and share the wave idioms next to it: wave_bcast, wave_incl_sum, wave_sum, wave_each.
// (Everything lives in an anonymous namespace: each .hip file that includes this header gets its own copy.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sj_stage2.h"

namespace {
using namespace sj;

static constexpr u64 TW_PAYLOAD = 0x00ffffffffffffffull;  // JSONVALUEMASK, parsed_json.go:27
static constexpr int TW_THREADS = 256, TW_ITEMS = 8, TW_TILE = TW_THREADS * TW_ITEMS;

__device__ __forceinline__ bool two_word_tag(u64 w) {
    const u32 t = (u32)(w >> 56);
    return t == '"' || t == 'l' || t == 'u' || t == 'd';
}

// ---- one wave: broadcast, sums, the lanes of a ballot in turn ---------------------------------------------------------------------
__device__ __forceinline__ u64 wave_bcast(u64 x, int j) { return (u64)__shfl((long long)x, j, 64); }  // lane j's x (j wave-uniform)
__device__ __forceinline__ u32 wave_bcast(u32 x, int j) { return (u32)__shfl((int)x, j, 64); }
__device__ __forceinline__ u64 wave_up(u64 x, int s) { return (u64)__shfl_up((long long)x, s, 64); }
__device__ __forceinline__ u32 wave_up(u32 x, int s) { return (u32)__shfl_up((int)x, s, 64); }
template <typename T>
__device__ __forceinline__ T wave_incl_sum(T x, int lane) {  // the sum over the lanes up to and including this one (u32 / u64)
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const T up = wave_up(x, s);
        if (lane >= s) x += up;
    }
    return x;
}
__device__ __forceinline__ u64 wave_sum(u64 x) {  // the sum over all 64 lanes, in every lane
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) x += (u64)__shfl_xor((long long)x, s, 64);
    return x;
}
// "The wave's long X, one after another": body(j) for every lane j whose `pred` holds, in lane order.  Every lane of the wave makes
// the call and every lane runs every body(j) -- j is wave-uniform, so a body may ballot and shuffle; it fetches lane j's values with
// wave_bcast and keeps what belongs to that lane under `if (lane == j)`.
template <typename F>
__device__ __forceinline__ void wave_each(bool pred, F body) {
    for (u64 todo = __ballot(pred); todo; todo &= todo - 1) body(__ffsll((unsigned long long)todo) - 1);
}

// The span walk: the words [v, v + nwords) of a tape by one wave, 64 per step.  body(i, w, in, raw) runs on every lane in every
// step -- wave-uniform, so a body may ballot and shuffle -- with i: the lane's word, relative to v; in: i < nwords; w: tape[v + i]
// (0 when !in); raw: the word is the second word of an entry, by the parity rule at the top of this file (undefined when !in).
// The step's anchors come from one ballot; the last anchor of a step is carried into the next.
// THE CALLER GUARANTEES that v is the first word of an entry (a record's root value, a row's value, a member): the word in front
// of the span then counts as an anchor at -1, whatever it is.  No `p >= 0` guard: a span that is one scalar -- "s" or a number, a
// two-word tag and no anchor inside -- has its word 1 told raw by exactly that anchor.
// (Tape: Arr<const u64> -- in the debug build every read goes through its checked operator[].)
template <typename Tape, typename F>
__device__ __forceinline__ void tw_walk_span(const Tape &tape, u64 v, u64 nwords, int lane, F body) {
    long long p_prev = -1;  // last anchor below the step, relative to v
    for (u64 g = 0; g < nwords; g += 64) {
        const u64 i = g + (u64)lane;
        const bool in = i < nwords;
        const u64 w = in ? tape[v + i] : 0;
        const u64 zm = ~__ballot(in && two_word_tag(w)) & __ballot(in);  // the anchors of the step
        const u64 zeros_below = zm & (lane ? (~0ull >> (64 - lane)) : 0ull);
        const long long p = zeros_below ? (long long)g + (63 - __builtin_clzll(zeros_below)) : p_prev;
        body(i, w, in, (((long long)i - p - 1) & 1) != 0);
        if (zm) p_prev = (long long)g + (63 - __builtin_clzll(zm));
    }
}

// block-wide exclusive scans over one value per thread (4 waves)
__device__ __forceinline__ long long block_excl_max(long long v, long long *s_w, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    long long incl = v;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const long long o = __shfl_up(incl, s, 64);
        if (lane >= s) incl = o > incl ? o : incl;
    }
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    long long before = -1;
    for (int w = 0; w < wave; w++) before = s_w[w] > before ? s_w[w] : before;
    long long ex = __shfl_up(incl, 1, 64);
    if (lane == 0) ex = -1;
    __syncthreads();
    return ex > before ? ex : before;
}
__device__ __forceinline__ unsigned long long block_excl_sum(unsigned long long v, unsigned long long *s_w, int tid,
                                                              unsigned long long *total) {
    const int lane = tid & 63, wave = tid >> 6;
    unsigned long long incl = v;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const unsigned long long o = (unsigned long long)__shfl_up((long long)incl, s, 64);
        if (lane >= s) incl += o;
    }
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    unsigned long long before = 0, tot = 0;
    for (int w = 0; w < TW_THREADS / 64; w++) {
        if (w < wave) before += s_w[w];
        tot += s_w[w];
    }
    if (total) *total = tot;
    __syncthreads();
    return before + incl - v;
}

// The anchor in front of the tile that starts at word tb, without the global pass (k_tw_last / k_tw_scan_last): the
// closest of the 64 words in front of the tile that is not a two-word tag.  -1: the tile is the first one; -2: none
// among the 64 (they are raw words that all look like string / number tags) -- the tile must then not classify
// anything (with a wrong anchor raw words would be read as tags and their neighbours as string offsets and lengths):
// it reports through a flag and the host repeats the walk with the global anchors.  Block-uniform result.
__device__ __forceinline__ long long tw_local_anchor(const u64 *tape, u64 tb, int tid, long long *s_carry) {
    if (tid < 64) {
        const bool have = tb >= 1 + (u64)tid;
        const bool c0 = have && !two_word_tag(tape[tb - 1 - (u64)tid]);
        const u64 b = __ballot(c0);
        if (tid == 0) *s_carry = b ? (long long)(tb - 1 - (u64)ctz64(b)) : (tb > 64 ? -2ll : -1ll);
    }
    __syncthreads();
    return *s_carry;
}

// In-place exclusive scan of a[0 .. n) by ONE 1024-thread block (the per-tile values of a walk: tens of thousands of
// elements).  Every wave owns a contiguous range and walks it 64 consecutive elements at a time (coalesced loads, a
// shuffle scan per step): pass 1 reduces the range, the 16 range totals meet in LDS, pass 2 scans and writes.
// MAX: running maximum (identity -1), else sum.  (The first version gave every THREAD a contiguous range: 64 different
// cache lines per load instruction, 180 us for 39 000 tiles.)
template <bool MAX>
__device__ __forceinline__ long long block1024_scan_array(long long *a, u32 n, long long *s_w /* [16] */, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    const long long id = MAX ? -1ll : 0ll;
    auto op = [](long long x, long long y) { return MAX ? (x > y ? x : y) : x + y; };
    const u32 per = ((n + 15u) / 16u + 63u) / 64u * 64u;
    const u32 lo = (u32)wave * per < n ? (u32)wave * per : n, hi = lo + per < n ? lo + per : n;
    long long acc = id;
    for (u32 c0 = lo; c0 < hi; c0 += 64 * 8) {  // (eight loads in flight: one at a time is a memory round trip per 64 entries)
        long long v8[8];
#pragma unroll
        for (int g = 0; g < 8; g++) {
            const u32 i = c0 + (u32)g * 64u + (u32)lane;
            v8[g] = i < hi ? a[i] : id;
        }
#pragma unroll
        for (int g = 0; g < 8; g++) acc = op(acc, v8[g]);
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) acc = op(acc, __shfl_xor(acc, s, 64));
    if (lane == 0) s_w[wave] = acc;
    __syncthreads();
    long long carry = id, total = id;
    for (int w = 0; w < 16; w++) {
        const long long x = s_w[w];
        if (w < wave) carry = op(carry, x);
        total = op(total, x);
    }
    for (u32 c0 = lo; c0 < hi; c0 += 64 * 8) {  // eight groups of 64 at a time: their loads are one round trip, not eight
        long long v8[8];
#pragma unroll
        for (int g = 0; g < 8; g++) {
            const u32 i = c0 + (u32)g * 64u + (u32)lane;
            v8[g] = i < hi ? a[i] : id;
        }
#pragma unroll
        for (int g = 0; g < 8; g++) {
            const u32 i = c0 + (u32)g * 64u + (u32)lane;
            long long incl = v8[g];
#pragma unroll
            for (int s = 1; s < 64; s <<= 1) {
                const long long o = __shfl_up(incl, s, 64);
                if (lane >= s) incl = op(o, incl);
            }
            long long ex = __shfl_up(incl, 1, 64);
            if (lane == 0) ex = id;
            if (i < hi) a[i] = op(carry, ex);
            carry = op(carry, __shfl(incl, 63, 64));
        }
    }
    __syncthreads();  // (s_w may be used again)
    return total;
}

// tile_last[tile] := the last anchor inside the tile that starts at word tile * TW_TILE (-1: none); s_w: one slot per wave
__device__ __forceinline__ void tw_tile_last(const u64 *tape, u64 n, long long *tile_last, long long *s_w) {
    const int tid = threadIdx.x;
    const u64 base = (u64)blockIdx.x * TW_TILE + (u64)tid * TW_ITEMS;
    long long last = -1;
#pragma unroll
    for (int k = 0; k < TW_ITEMS; k++)
        if (base + k < n && !two_word_tag(tape[base + k])) last = (long long)(base + k);
    // block maximum
    const int lane = tid & 63;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const long long o = __shfl_xor(last, s, 64);
        last = o > last ? o : last;
    }
    if (lane == 0) s_w[tid >> 6] = last;
    __syncthreads();
    if (tid == 0) {
        long long m = s_w[0];
        for (int w = 1; w < TW_THREADS / 64; w++) m = s_w[w] > m ? s_w[w] : m;
        tile_last[blockIdx.x] = m;
    }
}
__global__ __launch_bounds__(TW_THREADS) void k_tw_last(const u64 *tape, u64 n, long long *tile_last) {
    __shared__ long long s_w[TW_THREADS / 64];
    tw_tile_last(tape, n, tile_last, s_w);
}

// one block: tile_last[t] := the last anchor in front of tile t (exclusive running maximum)
__global__ __launch_bounds__(1024) void k_tw_scan_last(long long *tile_last, u32 tiles) {
    __shared__ long long s_w[16];
    block1024_scan_array<true>(tile_last, tiles, s_w, (int)threadIdx.x);
}

// one block: a0, a1, a2 [tiles] := their exclusive prefix sums, totals[k] := the sum of array k.  A null array is skipped and
// its total left as it is; null totals: nobody wants them.
__global__ __launch_bounds__(1024) void k_tw_scan_sums(unsigned long long *a0, unsigned long long *a1, unsigned long long *a2,
                                                       u32 tiles, unsigned long long *totals) {
    __shared__ long long s_w[16];
#pragma unroll 1
    for (int k = 0; k < 3; k++) {  // (one copy of the scan: three inlined ones spilled 84 bytes per lane under the 1024-thread bound)
        unsigned long long *const a = k == 0 ? a0 : (k == 1 ? a1 : a2);
        if (!a) continue;
        const long long t = block1024_scan_array<false>((long long *)a, tiles, s_w, (int)threadIdx.x);
        if (threadIdx.x == 0 && totals) totals[k] = (unsigned long long)t;
    }
}

// ---- exclusive prefixes over one value per record / row (query.hip, marshal.hip): tiles of 1024 elements (256 threads x 4
// consecutive ones), tile sums scanned by one block (k_tw_scan_sums), then applied: sums -> scan -> apply
static constexpr int QT = TW_THREADS, QI = 4, QTILE = QT * QI;
static_assert(QT == 256, "block_excl_sum / block_excl_max of sj_tapewalk.h scan the four waves of a 256-thread block");
// the thread's QI consecutive elements of the tile (16 or 32 bytes per thread); -> their sum
template <typename T>
__device__ __forceinline__ unsigned long long q_load4(const T *p, u32 n, T fill, T (&v)[QI]) {
    const u32 base = blockIdx.x * QTILE + threadIdx.x * QI;
    unsigned long long sum = 0;
#pragma unroll
    for (int k = 0; k < QI; k++) {
        v[k] = base + k < n ? p[base + k] : fill;
        sum += v[k];
    }
    return sum;
}
// The two tile steps of an exclusive prefix over a[0 .. n), around the one-block scan of the tile sums (k_tw_scan_sums):
// sums[tile] := the sum of the tile's elements;  dst[i] := sums[tile] (scanned) + the elements of the tile in front of i.
template <typename T>
__device__ __forceinline__ void tile_sums(const T *a, u32 n, unsigned long long *sums) {
    __shared__ unsigned long long s_w[QT / 64];
    T v[QI];
    unsigned long long tot = 0;
    (void)block_excl_sum(q_load4(a, n, (T)0, v), s_w, (int)threadIdx.x, &tot);
    if (threadIdx.x == 0) sums[blockIdx.x] = tot;
}
template <typename T>
__device__ __forceinline__ void tile_apply(const T *a, T *dst, u32 n, const unsigned long long *sums) {
    __shared__ unsigned long long s_w[QT / 64];
    const u32 base = blockIdx.x * QTILE + threadIdx.x * QI;
    T v[QI];
    unsigned long long pre = block_excl_sum(q_load4(a, n, (T)0, v), s_w, (int)threadIdx.x, nullptr) + sums[blockIdx.x];
#pragma unroll
    for (int k = 0; k < QI; k++) {
        if (base + k < n) dst[base + k] = (T)pre;
        pre += v[k];
    }
}

}  // namespace
