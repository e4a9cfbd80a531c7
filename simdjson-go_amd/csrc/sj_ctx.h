// sj_ctx.h -- host-side context behind the opaque sjhip_ctx of include/sjhip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "sj_device.h"
#include "sj_result.h"

namespace sj {
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    unsigned gen = 0;  // counts the allocations behind p (arena_reserve, sjhip_ctx_trim): "is this still the memory I prepared?"
};
}  // namespace sj

struct sjhip_ctx {
    int device = 0;
    hipStream_t stream = nullptr;      // stream all work is queued on
    hipStream_t own_stream = nullptr;  // created with the context
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    uint8_t *h_scratch = nullptr;      // 4 KiB pinned: state read-backs
    // small documents parsed from a host buffer (sjhip_parse): the last kernel of the chain also writes the stage-2 state,
    // the tape and Strings.B into this pinned block (over PCIe, no copy commands), and sjhip_fetch is two memcpy
    uint8_t *h_pack = nullptr;         // (res.packed(): it holds the result of the last parse)
    uint8_t *h_view = nullptr;         // sjhip_fetch_view of results that did not travel with the last launch (grows)
    size_t h_view_cap = 0;
    uint8_t *h_in = nullptr;           // sjhip_input_block: pinned block the caller reads its input into
    size_t h_in_cap = 0;
    uint8_t *h_stage = nullptr;        // pinned staging of sjhip_parse_batch: runs of small documents travel as one copy
    size_t h_stage_cap = 0;
    sj::DevBuf d_msg, d_pos, d_ws, d_kat, d_tape, d_strings, d_s2, d_s2z, d_aux;
    sj::DevBuf d_keyflag;              // SJHIP_FLAG_KEY_FLAGS: key flags of the string entries, for marshal.hip (res.key_flags())
    sj::DevBuf d_scol, d_stab;         // serializer with de-duplication: the string column, the hash table
    // shared by the filter (query.hip: work arrays, filtered tape / Strings.B), the serializer and MarshalJSON: res says whose they are
    sj::DevBuf d_q, d_qtape, d_qstrings;
    sj::DevBuf d_col;                  // the string column of the last sjhip_extract_path_strings (query.hip): offsets, status, bytes
    sj::DevBuf d_list;                 // the list column of the last sjhip_extract_path_list[_strings] (query.hip), apart from d_col
    // the table of the last sjhip_extract_table (query.hip): the numeric columns and the offsets / statuses of the string columns
    // (laid out before the walk that fills them), and the string columns' bytes (whose size the walk finds out)
    sj::DevBuf d_table, d_tabledata;
    sj::DevBuf d_rows;                 // the row selection of the last sjhip_select_rows (query.hip): row offsets, status, row index
    // the grouping of the last sjhip_group_path (query.hip): the dictionary, first_row, group_rows, codes, key statuses, aggregates
    sj::DevBuf d_group;
    sj::DevBuf d_order;                // the order of the last sjhip_order_path (query.hip): row numbers, keys and statuses by rank
    // the row parents of the last sjhip_unnest_rows (query.hip): parent offsets, parent statuses, the parent of every new row --
    // and, behind them, the new row index on its way into d_rows (the old one is read while it is written)
    sj::DevBuf d_parents;
    // the row schema of the last sjhip_row_schema (query.hip): name offsets, first rows, counts per name and type, the names' bytes
    // (d_schema), and the work arrays of its second half, sized by the members the first half counted (d_schema_work: d_kat holds
    // the member walk's arrays, which that half still reads, and a second reservation would move it)
    sj::DevBuf d_schema, d_schema_work;
    // the set of the sjhip_where_path_in call at work (query.hip): the uploaded values, their hashes and the table over them.  Working
    // data, not a product: nothing refers to it once the call has returned
    sj::DevBuf d_in;
    unsigned ws_clean_gen = 0;         // d_ws.gen of the allocation that has been zeroed for stage 1 (0: none; stage1_enqueue)
    sj::S1Ws s1ws;                     // ... and its launch count (sj_device.h: a launch cleans up for the next one)
    // queued stage-1 messages that wait for their launch (api.hip: the queue runs up to S1_GROUP_MAX messages of one mode as one
    // launch): s1q_n of them, s1q_tiles descriptors together; stage1_queue_flush launches them
    sj::S1QMsg s1q[sj::S1_GROUP_MAX];
    int s1q_n = 0, s1q_nd = 0;
    size_t s1q_tiles = 0;
    unsigned s1_par = 0;               // control slot of the last stage-1 launch (Stage1State::c[]: stage 2 reads has_starter there)
    sj::Stage1State s1;                // last stage-1 state (host copy)
    // the tape and Strings.B in d_tape / d_strings (what sjhip_fetch copies): of the last parse, or of the last sjhip_deserialize
    size_t tape_len = 0, strings_len = 0;
    sj::ResultState res;          // what the device holds of the last parse and of the products derived from it (sj_result.h)
    uint32_t q_records = 0;       // record-separating newline runs of that parse (records - 1)
    size_t des_msg_len = 0;       // last sjhip_deserialize: length of pj.Message (in d_msg)
    // a parse between its two phases (sjhip_parse_shard_begin / _finish: res.pending())
    int p_deferred = 0;   // stage 1's result has not been collected yet (small documents: one synchronisation per parse)
    int p_collected = 0;  // ... but a shard's phase 1 has: its sizes and stage 1's verdict arrive with one synchronisation (parse_begin)
    int p_no_defer = 0;   // the deferred run met more tokens than its layout holds: this parse takes the synchronous path
    uint32_t p_density_q = 0;  // tokens per KiB of the context's last successful parse (+1), 0: none yet -- a large document is
                               // then parsed without the host round trip between the stages, laid out for that density + 1/16 (or what the arenas hold)
    int p_dense = 0;      // sticky: a document of this context was denser than one token per four bytes -- later deferred
                          // parses are laid out for one token per byte instead of paying the second parse again
    uint8_t p_last = 0;   // ... its caller-supplied last byte
    int p_have_last = 0;
    size_t p_nlay = 0;    // the token count the stage-2 arrays were laid out for (>= p_n)
    const void *p_msg = nullptr;
    size_t p_len = 0, p_n = 0;
    uint32_t p_flags = 0;
    void *p_aux = nullptr;
    uint8_t *p_kind = nullptr;  // token kinds of the pending parse (behind the positions in d_pos)
    // an ND message beyond 4 GiB - 64 is parsed shard by shard by a multi handle the context owns (multi_api.hip
    // parse_nd_big); the merged result waits there for sjhip_fetch
    struct sjhip_multi *big = nullptr;  // (res.sharded(): it holds the last result)
    char err[256];
};

namespace sj {
// Pinned host memory of the library: portable (every device context may use it, not only the one that was current when
// it was allocated -- streams and multi handles own contexts on several devices) and mapped (kernels of any of them
// write results straight into it: the stage-1 verdict word, k_pack, the batch end check).
inline hipError_t pinned_alloc(void **p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocPortable | hipHostMallocMapped); }
void ctx_set_error(sjhip_ctx *ctx, const char *fmt, ...);
// SJHIP_ERR_ARG of a call that needs a parse result on the device and finds none (`follows`: "queries follow", "sjhip_x follows")
int no_result(sjhip_ctx *ctx, const char *follows);
// ... and of one that works on the whole result of one context (the filter, the serializer): a sharded result has its own text
int no_whole_result(sjhip_ctx *ctx, const char *call, const char *follows);
// the return code of a call that has just published a product: an internal error if there was no result to publish it on
int published(sjhip_ctx *ctx, bool ok);
// Launches the queued stage-1 messages that still wait for company (api.hip).  The one hook of everything that must not
// overtake them: a parse (begin_parse), a stage-1 entry point, _wait, and whatever changes or frees the stream or the arenas.
// A failure is left in the context; the messages' records then stay "left no result".
int stage1_queue_flush(sjhip_ctx *ctx);
// a parse entry point, before anything that can return: the last result and everything derived from it are gone
inline void begin_parse(sjhip_ctx *ctx) {
    if (ctx->s1q_n) (void)stage1_queue_flush(ctx);
    ctx->res.begin_parse();
    ctx->tape_len = ctx->strings_len = 0;
}
int ctx_hip_fail(sjhip_ctx *ctx, hipError_t e, const char *what);
int arena_reserve(sjhip_ctx *ctx, DevBuf &b, size_t bytes);
// a failed HIP call ends the calling function with the error left in `ctx` (the name in scope at the call)
#define HIPCHK(call, what)                                              \
    do {                                                                \
        hipError_t e_ = (call);                                         \
        if (e_ != hipSuccess) return ::sj::ctx_hip_fail(ctx, e_, what); \
    } while (0)
// The work areas of an arena: 256-byte aligned slices off a base pointer, one after another; `used` is what to reserve.  A layout
// written once as a function of a Carve is run twice: without a base for the size, then on the reserved arena.
struct Carve {
    char *base;
    size_t used = 0;
    explicit Carve(void *b = nullptr) : base((char *)b) {}
    template <typename T>
    T *take(size_t count) {
        T *p = (T *)(base + used);
        used += (count * sizeof(T) + 255) / 256 * 256;
        return p;
    }
};
// the row selection of a part in its d_rows (query.hip writes it; marshal.hip reads the row index): row offsets over the n records
// the selection ran over, their statuses, the tape index of every row's value
struct RowsOut { uint64_t *off, *index; uint8_t *status; };
inline size_t rows_layout(Carve c, size_t n, size_t rows, RowsOut *o) {
    o->off = c.take<uint64_t>(n + 1);
    o->status = c.take<uint8_t>(n);
    o->index = c.take<uint64_t>(rows);
    return c.used;
}
int parse_packed(sjhip_ctx *ctx, size_t len, uint32_t flags, uint8_t last_byte, int have_last, size_t *tape_len,
                 size_t *strings_len);  // parse_api.hip
int parse_nd_big(sjhip_ctx *ctx, const uint8_t *msg, size_t len, uint32_t flags, bool d_resident, size_t shard_bytes,
                 size_t *tape_len, size_t *strings_len, size_t *msg_off, size_t *msg_len);  // multi_api.hip
int fetch_nd_big(sjhip_ctx *ctx, uint64_t *tape_dst, uint8_t *strings_dst);
void release_nd_big(sjhip_ctx *ctx);
size_t nd_big_device_bytes(const sjhip_ctx *ctx);  // arenas of the shard contexts of a sharded ND parse
// the shards of the merged result of parse_nd_big, in document order (empty shards have no context to look at: null)
int nd_big_shards(const sjhip_ctx *ctx);
sjhip_ctx *nd_big_shard(const sjhip_ctx *ctx, int k);
// The contexts whose device-resident results make up the last parse of `ctx`, in document order: the context itself, or -- after
// parse_nd_big -- the contexts of its shards that hold something.  On the heap, as many as there are (no thread_local array: a
// library linked at start-up carries its thread_local storage in the static TLS block of every thread of the process).
std::vector<sjhip_ctx *> result_parts(sjhip_ctx *ctx);
int stage1_enqueue(sjhip_ctx *ctx, const void *d_msg, size_t len, int ndjson, void *d_pos, size_t pos_cap, void *str_aux,
                   uint8_t *d_kind, void *zero2, size_t zero2_bytes, unsigned long long *host_rec = nullptr);
// host_rec: the launch's record in pinned host memory (S1_HOST_WORDS words; null: the context's own at h_scratch)
int stage1_collect(sjhip_ctx *ctx, size_t len, uint8_t last_byte, int have_last, size_t *n, int *ok,
                   const unsigned long long *host_rec = nullptr);
int stage1_run_device(sjhip_ctx *ctx, const void *d_msg, size_t len, int ndjson, void *d_pos, size_t pos_cap,
                      uint8_t last_byte, int have_last, size_t *n, int *ok, void *str_aux = nullptr, uint8_t *d_kind = nullptr,
                      void *zero2 = nullptr, size_t zero2_bytes = 0);
}  // namespace sj
