// sj_sort.h -- the one stable least-significant-digit radix sort of (key, row) pairs on the device (query.hip: the grouping sorts the
// rows by their uint32 code, the ordering by their uint64 key): its geometry and its pass plans, plain C++ under SJ_HD so that the
// CPU build of a test program can run them (host_selftest.cpp); under hipcc, the kernels and the host driver as well.
//
// SORT_RADIX_BITS per pass, tiles of SORT_TILE pairs (SORT_THREADS threads, SORT_ROUNDS pairs each, taken in rounds so that the
// order inside a tile is the input order), at most SORT_PASSES passes.  A pass is: per tile a digit histogram (k_q_sort_hist), an
// exclusive scan of the digit-major histograms (k_q_sort_scan_sums -> k_tw_scan_sums -> k_q_sort_scan_apply), and a scatter
// (k_q_sort_scatter) whose rank inside the tile is the input order: wave ballots match equal digits, the waves and the rounds of a
// tile are taken in order.  No contended atomics in global memory anywhere.
#pragma once
#include "sj_chunk.h"  // SJ_HD, u8 / u32 / u64

namespace sj {

static constexpr int SORT_RADIX_BITS = 8, SORT_RADIX = 1 << SORT_RADIX_BITS, SORT_PASSES = 64 / SORT_RADIX_BITS;
static constexpr int SORT_THREADS = 256, SORT_ROUNDS = 4, SORT_TILE = SORT_THREADS * SORT_ROUNDS;
static_assert(SORT_RADIX == SORT_THREADS, "thread d of a sort block owns digit d");

// The pass plan: bit p is set iff the sort takes the pass over digit p (bits 8p .. 8p + 7 of the key).
// The ordering -- and_ / or_: the AND and the OR of all keys that are sorted; a bit that is equal in both is equal in every key,
// and a digit of such bits orders nothing.  Equal keys (and a single key) take no pass.
SJ_HD u32 order_pass_mask(u64 and_, u64 or_) {
    const u64 varying = and_ ^ or_;
    u32 mask = 0;
    for (int p = 0; p < SORT_PASSES; p++)
        if ((varying >> (SORT_RADIX_BITS * p)) & (u64)(SORT_RADIX - 1)) mask |= 1u << p;
    return mask;
}
// The grouping -- the codes 0 .. groups (code `groups`: the rows without a key, which sort behind every group): the low digits, as
// many as `groups` has, at least one.
SJ_HD u32 group_pass_mask(u64 groups) {
    u32 p = 1;
    while (p < (u32)SORT_PASSES && (groups >> (SORT_RADIX_BITS * p)) != 0) p++;
    return (1u << p) - 1u;
}

}  // namespace sj

#if defined(__HIPCC__)
#include "sj_bounds.h"
#include "sj_ctx.h"       // Carve
#include "sj_tapewalk.h"  // QT, QTILE, tile_sums / tile_apply, k_tw_scan_sums

namespace {
using namespace sj;

template <typename K>
struct QSort {
    u32 n, shift;  // n: the pairs that are sorted
    Arr<const K> keys_in;
    Arr<const u32> rows_in;  // null: position i is row i (a first pass without row numbers)
    Arr<K> keys_out;
    Arr<u32> rows_out;
    Arr<u32> hist;  // [SORT_RADIX * tiles] digit-major: entry d * tiles + t
};
// the lanes of the wave whose digit equals this lane's (valid lanes only; undefined on the others), by one ballot per digit bit
__device__ __forceinline__ u64 sort_match_digit(bool valid, u32 d) {
    u64 m = __ballot(valid);
#pragma unroll
    for (int b = 0; b < SORT_RADIX_BITS; b++) {
        const bool bit = (d >> b) & 1u;
        const u64 bb = __ballot(valid && bit);
        m &= bit ? bb : ~bb;
    }
    return m;
}
template <typename K>
__global__ __launch_bounds__(SORT_THREADS) void k_q_sort_hist(QSort<K> s) {
    __shared__ u32 s_h[SORT_RADIX];
    const int tid = threadIdx.x, lane = tid & 63;
    s_h[tid] = 0;
    __syncthreads();
    for (int k = 0; k < SORT_ROUNDS; k++) {
        const u32 i = blockIdx.x * SORT_TILE + k * SORT_THREADS + tid;
        const bool valid = i < s.n;
        const u32 d = valid ? (u32)(s.keys_in[i] >> s.shift) & (SORT_RADIX - 1) : 0u;
        const u64 m = sort_match_digit(valid, d);
        if (valid && (m & ((1ull << lane) - 1)) == 0) atomicAdd(&s_h[d], (u32)__popcll(m));  // (LDS: the lowest lane of every digit)
    }
    __syncthreads();
    s.hist[(u64)tid * gridDim.x + blockIdx.x] = s_h[tid];
}
__global__ __launch_bounds__(QT) void k_q_sort_scan_sums(Arr<u32> a, u32 m, unsigned long long *tiles) { tile_sums(arr_raw(a), m, tiles); }
__global__ __launch_bounds__(QT) void k_q_sort_scan_apply(Arr<u32> a, u32 m, unsigned long long *tiles) {
    tile_apply(arr_raw(a), arr_raw(a), m, tiles);
}
template <typename K>
__global__ __launch_bounds__(SORT_THREADS) void k_q_sort_scatter(QSort<K> s) {
    __shared__ u32 s_base[SORT_RADIX], s_cnt[SORT_THREADS / 64][SORT_RADIX];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    s_base[tid] = s.hist[(u64)tid * gridDim.x + blockIdx.x];  // where the tile's pairs of digit `tid` begin
    for (int k = 0; k < SORT_ROUNDS; k++) {
#pragma unroll
        for (int w = 0; w < SORT_THREADS / 64; w++) s_cnt[w][tid] = 0;
        __syncthreads();
        const u32 i = blockIdx.x * SORT_TILE + k * SORT_THREADS + tid;
        const bool valid = i < s.n;
        const K key = valid ? s.keys_in[i] : (K)0;
        const u32 row = valid ? (s.rows_in ? s.rows_in[i] : i) : 0u;
        const u32 d = (u32)(key >> s.shift) & (SORT_RADIX - 1);
        const u64 m = sort_match_digit(valid, d);
        const u32 rank = (u32)__popcll(m & ((1ull << lane) - 1));  // equal digits in front of this lane in its wave
        if (valid && rank == 0) s_cnt[wave][d] = (u32)__popcll(m);
        __syncthreads();
        if (valid) {
            u32 pos = s_base[d] + rank;
            for (int w = 0; w < SORT_THREADS / 64; w++)
                if (w < wave) pos += s_cnt[w][d];
            s.keys_out[pos] = key;
            s.rows_out[pos] = row;
        }
        __syncthreads();
        u32 add = 0;
#pragma unroll
        for (int w = 0; w < SORT_THREADS / 64; w++) add += s_cnt[w][tid];
        s_base[tid] += add;  // (thread `tid` alone touches entry `tid` until the next round's barrier)
    }
}

// ---- host: the buffers of a sort of up to `cap` pairs in an arena, and its passes on a stream -----------------------------------------
template <typename K>
struct SortWork {
    K *keys[2];    // [cap] each; the input lies in keys[0] / rows[0]
    u32 *rows[2];  // [cap] each
    u32 *hist;     // [SORT_RADIX * sort_tiles(cap)]
    unsigned long long *hist_tiles;
};
static u32 sort_tiles(u32 n) { return (n + SORT_TILE - 1) / SORT_TILE; }
template <typename K>
static void sort_carve(Carve &c, u32 cap, SortWork<K> *w) {
    const u32 hist_n = (u32)SORT_RADIX * sort_tiles(cap);
    for (int k = 0; k < 2; k++) w->keys[k] = c.take<K>(cap), w->rows[k] = c.take<u32>(cap);
    w->hist = c.take<u32>(hist_n);
    w->hist_tiles = c.take<unsigned long long>((hist_n + QTILE - 1) / QTILE);
}
// The first n of the cap pairs ordered by key, stably, over the digits of `mask`: the j-th pass taken reads keys / rows [j & 1] and
// writes [(j + 1) & 1].  has_rows false: pair i is row i, and rows[0] is not read.  Returns the buffer the result lies in.
template <typename K>
static int sort_enqueue(hipStream_t st, u32 n, u32 cap, u32 mask, bool has_rows, const SortWork<K> &w) {
    const u32 stiles = sort_tiles(n), hist_n = (u32)SORT_RADIX * stiles, htiles = (hist_n + QTILE - 1) / QTILE;
    unsigned long long *const none = nullptr;
    int at = 0;
    for (u32 p = 0; p < (u32)SORT_PASSES; p++) {
        if (!(mask >> p & 1u)) continue;
        QSort<K> s;
        s.n = n, s.shift = p * SORT_RADIX_BITS;
        K *const keys_in = w.keys[at], *const keys_out = w.keys[at ^ 1];
        u32 *const rows_in = has_rows ? w.rows[at] : nullptr, *const rows_out = w.rows[at ^ 1];
        s.keys_in = SJ_ARR(keys_in, cap, A_SORT);
        s.rows_in = SJ_ARR(rows_in, has_rows ? cap : 0, A_SORT);
        s.keys_out = SJ_ARR(keys_out, cap, A_SORT);
        s.rows_out = SJ_ARR(rows_out, cap, A_SORT);
        s.hist = SJ_ARR(w.hist, hist_n, A_SORT_HIST);
        hipLaunchKernelGGL(k_q_sort_hist<K>, dim3(stiles), dim3(SORT_THREADS), 0, st, s);
        hipLaunchKernelGGL(k_q_sort_scan_sums, dim3(htiles), dim3(QT), 0, st, s.hist, hist_n, w.hist_tiles);
        hipLaunchKernelGGL(k_tw_scan_sums, dim3(1), dim3(1024), 0, st, w.hist_tiles, none, none, htiles, none);
        hipLaunchKernelGGL(k_q_sort_scan_apply, dim3(htiles), dim3(QT), 0, st, s.hist, hist_n, w.hist_tiles);
        hipLaunchKernelGGL(k_q_sort_scatter<K>, dim3(stiles), dim3(SORT_THREADS), 0, st, s);
        at ^= 1, has_rows = true;
    }
    return at;
}

}  // namespace
#endif
