/*
 * sjhip.h -- C ABI of libsjhip: the MI355X (gfx950) engine behind the simdjson-go
 * Parse()/ParseND() hot path.
 *
 * This is the drop-in boundary.  The reference selects its backend with build tags
 * (simdjson_amd64.go:1 vs simdjson_other.go:1); a backend has to provide SupportedCPU,
 * Parse, ParseND and ParseNDStream (simdjson_other.go:29-76), all of which funnel into
 *     (*internalParsedJson).parseMessage(msg []byte, ndjson bool) error      parse_json_amd64.go:52
 * whose only outputs are pj.Message (TrimSpace'd alias of the input), pj.Tape []uint64 and
 * pj.Strings.B []byte.  The Go shim (simdjson-go_amd/go/simdjson_hip.go)
 * binds exactly the functions below through cgo; the Python mirror (sjhip package) binds the
 * same symbols through ctypes.
 *
 * Conventions (they mirror the Go<->asm seam of find_subroutines_amd64.go):
 *   - plain pointers + explicit sizes; the library never retains a caller pointer after the
 *     call returns (cgo rule), hence the two-call parse/fetch protocol;
 *   - one sjhip_ctx per concurrent parse (it owns a HIP stream and device arenas that are
 *     recycled across calls -- the role of the reference's `reuse *ParsedJson`);
 *   - functions return 0 on success, SJHIP_ERR_* otherwise; sjhip_last_error() explains.
 */
#ifndef SJHIP_H
#define SJHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sjhip_ctx sjhip_ctx;

/* flags for sjhip_parse: parse_json_amd64.go:58-62 (ndjson) and options.go:13 (WithCopyStrings) */
#define SJHIP_FLAG_NDJSON 1u
#define SJHIP_FLAG_COPY_STRINGS 2u
/* The caller is going to call sjhip_marshal_json on this result: the parse also leaves, on the device, one byte per
 * string entry of the tape saying whether it is an object key (the parser knows: the token behind it is ':'), and
 * MarshalJSON neither recovers that from the token array (three launches) nor needs its counting pass: it becomes one
 * pass over the tape (marshal.hip).  No effect on the result of the parse. */
#define SJHIP_FLAG_KEY_FLAGS 4u

/* return codes */
#define SJHIP_OK 0
#define SJHIP_ERR_STAGE1 1  /* "Failed to find all structural indices for stage 1" parse_json_amd64.go:93 */
#define SJHIP_ERR_STAGE2 2  /* "Bad parsing while executing stage 2"               parse_json_amd64.go:81 */
#define SJHIP_ERR_NODEVICE 3 /* "Host CPU does not meet target specs" analogue     simdjson_amd64.go:43  */
#define SJHIP_ERR_TOOBIG 4  /* plain stage 1: message longer than 4 GiB - 64 (it hands out uint32 positions); whole parse: more than
                             * 2^32 tokens / tape words / bytes of Strings.B, tokens 4 GiB apart, or a message beyond 256 GiB */
#define SJHIP_ERR_ARG 5
#define SJHIP_STREAM_FULL 6  /* sjhip_stream_acquire: every slot holds a block: take a result first */
#define SJHIP_STREAM_EMPTY 7 /* sjhip_stream_next: nothing submitted is outstanding */
#define SJHIP_ERR_STREAM_CLOSED 8 /* the stream has delivered an error: it accepts and delivers nothing more */
#define SJHIP_ERR_HIP (-1)  /* a HIP runtime call failed */

/* ---- backend presence: replaces SupportedCPU() (simdjson_amd64.go:37) -------------------- */
int sjhip_supported(void);      /* 1 iff a gfx950 device is visible */
int sjhip_device_count(void);

/* ---- context ------------------------------------------------------------------------------ */
sjhip_ctx *sjhip_ctx_create(int device);          /* NULL if the device is unusable */
void sjhip_ctx_destroy(sjhip_ctx *ctx);
const char *sjhip_last_error(const sjhip_ctx *ctx);
/* run the context's work on an existing HIP stream (e.g. torch's current stream); NULL = own stream */
int sjhip_ctx_set_stream(sjhip_ctx *ctx, void *hip_stream);
/* A context's arenas only grow (they are the capacity a recycled `reuse *ParsedJson` carries, simdjson_amd64.go:46-51),
 * sized by the largest message it has parsed.  sjhip_ctx_device_bytes reports what it holds on the device right now;
 * sjhip_ctx_trim gives all of it back (device arenas, the pinned result blocks, the contexts of a sharded ND parse) and
 * drops the resident result -- a pool calls it on a context that has just parsed an unusually large message.  The
 * next parse allocates what it needs. */
size_t sjhip_ctx_device_bytes(const sjhip_ctx *ctx);
int sjhip_ctx_trim(sjhip_ctx *ctx);

/* ---- whole parse: replaces parseMessage (parse_json_amd64.go:52-127) ------------------------
 * msg is a HOST buffer.  The library applies bytes.TrimSpace (parse_json_amd64.go:55) and reports
 * the trimmed window so that the caller can alias pj.Message = msg[msg_off : msg_off+msg_len].
 * On SJHIP_OK the tape/strings stay on the device until sjhip_fetch copies them into
 * caller-owned memory of at least tape_len*8 / strings_len bytes.
 * A parse call on a context (this one, sjhip_parse_device, sjhip_parse_batch[_device]), successful or not, drops the
 * previous result and everything derived from it. */
int sjhip_parse(sjhip_ctx *ctx, const uint8_t *msg, size_t len, uint32_t flags, size_t *tape_len,
                size_t *strings_len, size_t *msg_off, size_t *msg_len);
int sjhip_fetch(sjhip_ctx *ctx, uint64_t *tape_dst, uint8_t *strings_dst);
/* The same result WITHOUT the copy into caller memory: *tape / *strings point at tape_len words / strings_len bytes in
 * pinned host memory that the context owns, valid until the next call that parses on this context (or destroys it).
 * This is what `reuse *ParsedJson` means in the reference (simdjson_amd64.go:46-51: the arrays of the recycled
 * ParsedJson are overwritten by the next parse): a binding that keeps one context per recycled ParsedJson hands these
 * pointers out as pj.Tape / pj.Strings.  A small document parsed by sjhip_parse is
 * already there (its last kernel wrote the result over PCIe); anything else is copied device -> pinned block here
 * (the block grows on demand, SJHIP_ERR_TOOBIG beyond SJHIP_VIEW_LIMIT_BYTES, default 4 GiB: use sjhip_fetch).
 * Either pointer is NULL when its length is 0. */
int sjhip_fetch_view(sjhip_ctx *ctx, const uint64_t **tape, const uint8_t **strings);

/* A pinned host block of at least `bytes` bytes owned by the context, for callers that can read their input (a file, a
 * socket) straight into it -- the role of the reference's tmpPool blocks in ParseNDStream (simdjson_amd64.go:127-135) for
 * a single Parse: sjhip_parse(ctx, block, len, ...) then copies host -> device at the pinned rate (twitter.json: 19
 * instead of 28 us).  Valid until the next sjhip_input_block call with a larger size, sjhip_ctx_trim or destroy. */
uint8_t *sjhip_input_block(sjhip_ctx *ctx, size_t bytes);

/* Same parse on a message that is already resident in device memory (already trimmed). Used by
 * bench.py (inputs in HBM before the timed region) and by the multi-GPU shard path. */
int sjhip_parse_device(sjhip_ctx *ctx, const void *d_msg, size_t len, uint32_t flags, size_t *tape_len,
                       size_t *strings_len);

/* ---- one NDJSON shard of a larger document: the multi-GPU ParseND path -------------------------------
 * ParseND's records are independent (simdjson_amd64.go:82, and ParseNDStream parses 10 MiB blocks on their own,
 * :156-192), so a document cut at record boundaries is parsed shard by shard, one shard per GPU.  The merged
 * ParsedJson is the concatenation of the shard tapes / Strings.B, provided every index a shard's tape stores is
 * rebased by where the shard starts in the merged Tape / Strings.B / Message.  Those three offsets are the
 * exclusive prefix sums of the preceding shards' sizes -- the only data the shards exchange (8+8 bytes per rank).
 *   begin : stage 1 + stage 2 up to the scan; returns this shard's tape_len / strings_len (message already on
 *           the device, trimmed, starting at a record boundary)
 *   ...   : all-gather the sizes (RCCL), compute the bases
 *   finish: emits tape and Strings.B with the rebased indices; then sjhip_fetch as usual.
 *
 * The window of a shard is its cut range inside the TrimSpace window of the whole message, without the JSON whitespace
 * (space, \t, \n, \r) at its ends and nothing else: the reference trims the message once, every other byte between two
 * records is parsed as it stands (and rejected).  SJHIP_FLAG_INNER_SHARD (sjhip_parse_shard_begin only) says that a later
 * shard holds something, i.e. that the message does not end with this window: "the last structural is a closing bracket"
 * (stage1_find_marks_amd64.go:120-129) is asked of the end of the message, so a window that ends otherwise -- a stray byte
 * or a scalar behind its last record, a record broken across a newline -- and has no other stage-1 fault fails with
 * SJHIP_ERR_STAGE2, the verdict of the whole message, not with SJHIP_ERR_STAGE1. */
#define SJHIP_FLAG_INNER_SHARD 8u
int sjhip_parse_shard_begin(sjhip_ctx *ctx, const void *d_msg, size_t len, uint32_t flags, size_t *tape_len,
                            size_t *strings_len);
int sjhip_parse_shard_finish(sjhip_ctx *ctx, uint64_t tape_base, uint64_t strings_base, uint64_t msg_base);
/* ---- ParseND over several GPUs in one call (simdjson_amd64.go:82-94 is one call in one process) -------------------
 * A handle owns one context per entry of `devices` (NULL / 0 = every visible device; a device may be listed more than
 * once: several shards on one GPU).  sjhip_parse_nd_multi cuts the HOST message at record boundaries into one shard per
 * entry, runs the two-phase shard parse above on all of them in parallel (one host thread per shard; the sizes meet in
 * a host prefix sum of 16 bytes per shard -- no device collective) and sjhip_fetch_multi copies every shard's piece
 * straight into its slice of the caller's Tape / Strings.B: the result is bit for bit the ParsedJson of ParseND on
 * the whole message.  A stage-1 failure of any shard wins over stage-2 failures (parse_json_amd64.go:97-105,123-126). */
typedef struct sjhip_multi sjhip_multi;
sjhip_multi *sjhip_multi_create(const int *devices, int n);
void sjhip_multi_destroy(sjhip_multi *m);
int sjhip_multi_shards(const sjhip_multi *m);
/* the device that holds the tape of shard `shard` after a parse, as the HIP runtime reports it for that allocation
 * (hipPointerGetAttributes), -1 if the shard has parsed nothing yet: lets a caller (and the tests) see that the shards
 * really sit on the devices they were asked for */
int sjhip_multi_shard_device(const sjhip_multi *m, int shard);
const char *sjhip_multi_last_error(const sjhip_multi *m);
int sjhip_parse_nd_multi(sjhip_multi *m, const uint8_t *msg, size_t len, uint32_t flags, size_t *tape_len,
                         size_t *strings_len, size_t *msg_off, size_t *msg_len);
int sjhip_fetch_multi(sjhip_multi *m, uint64_t *tape_dst, uint8_t *strings_dst);
/* ---- many documents, one launch set (the goroutine-per-Parse shape of benchmarks_test.go:60-75, batched) ------------
 * The documents are packed into one device message -- each trimmed like Parse() trims it (parse_json_amd64.go:55),
 * separated by '\n', a raw '\n' INSIDE a document replaced by '\r' (whitespace either way outside strings, the same
 * stage-1 error inside one; "1\n2" stays the error it is in Parse()) -- and parsed as one ND document.  The result is
 * what ParseND of that message returns: document i is root i of the tape (Iter.Advance walks them), all string words
 * point into one Strings.B; sjhip_fetch and every query / serializer call work on it.  An empty document or any invalid
 * one fails the whole batch with the code Parse() of that document returns (stage 1 before stage 2) -- including the
 * end-of-message rule of stage 1 (the last structural must close a container, stage1_find_marks_amd64.go:115-129), to
 * which every document is held while the batch is packed: a scalar, a truncated or an all-whitespace document is
 * SJHIP_ERR_STAGE1 wherever it stands.  Needs SJHIP_FLAG_COPY_STRINGS.
 * sjhip_parse_batch_device: the documents lie in ONE device buffer at offs[i] (lens[i] bytes, taken untrimmed: JSON
 * whitespace around a document is whitespace of its record). */
int sjhip_parse_batch(sjhip_ctx *ctx, const uint8_t *const *msgs, const size_t *lens, size_t n, uint32_t flags,
                      size_t *tape_len, size_t *strings_len);
int sjhip_parse_batch_device(sjhip_ctx *ctx, const void *d_buf, const size_t *offs, const size_t *lens, size_t n,
                             uint32_t flags, size_t *tape_len, size_t *strings_len);
/* bytes.TrimSpace exactly as parseMessage applies it (parse_json_amd64.go:55); for hosts that are not Go */
void sjhip_trim_space(const uint8_t *msg, size_t len, size_t *off, size_t *out_len);

/* ---- queries on the device-resident result (no reference counterpart in the parser: they replace what callers do with
 * Iter / Object.FindKey on the host, ndjson_test.go:421-471, parsed_object.go:97-138, README.md:226-269) ------------
 * Both work on the result of the last successful sjhip_parse / sjhip_parse_device of `ctx` (still on the device).
 * Results larger than one context (round 6): after an ND message beyond 4 GiB -- parsed shard by shard, every shard resident on
 * its own context -- sjhip_count_where, the path / key-set queries below and sjhip_marshal_json run shard by shard and return
 * what they return on the merged ParsedJson (counts added up, per-record answers in document order holding indexes of the MERGED
 * tape, texts joined with the newline between two records), like the reference's Iter on any ParsedJson (parsed_json.go:96,125,833);
 * sjhip_filter_where and sjhip_serialize need the result of one context and say so (SJHIP_ERR_ARG).
 * A record matches when its root value is an object whose FIRST member with key == `key` (top level only, like
 * Object.FindKey) has a string value == `value` (compared after unescaping) -- the reference's countWhere.
 *   count_where : number of matching records; 8 bytes cross PCIe.
 *   filter_where: compacts the matching records into a new self-contained (Tape, Strings.B) on the device, identical
 *                 to ParseND of the document made of the matching lines (root chain re-linked, container / string
 *                 offsets rebased); sjhip_fetch_filtered copies it to the host.  Needs SJHIP_FLAG_COPY_STRINGS.
 *                 (Any other predicate, and rows inside arrays: sjhip_where_path + sjhip_filter_rows below.) */
int sjhip_count_where(sjhip_ctx *ctx, const uint8_t *key, size_t klen, const uint8_t *value, size_t vlen, uint64_t *count);
int sjhip_filter_where(sjhip_ctx *ctx, const uint8_t *key, size_t klen, const uint8_t *value, size_t vlen,
                       uint64_t *n_records, size_t *tape_len, size_t *strings_len);
int sjhip_fetch_filtered(sjhip_ctx *ctx, uint64_t *tape_dst, uint8_t *strings_dst);

/* Paths, typed values and key sets on the same device-resident result (round 5).  A path is n_keys keys, concatenated in
 * `keys`, key j being key_lens[j] bytes long (at most 16 keys, 1024 bytes together); every call evaluates it on the root
 * value of EVERY record (one record for a plain document) with the semantics of the reference's host API:
 *   sjhip_find_path        Iter.FindElement(path...) (parsed_json.go:833-865) = Object.FindPath (parsed_object.go:256-313):
 *                          into the root and into objects, not into arrays; at every level the first member with the key
 *                          wins.  index_out[r] = tape index of the element's value (tape[index] is its tag word), or
 *                          SJHIP_PATH_NOT_FOUND (ErrPathNotFound) or SJHIP_PATH_NOT_OBJECT (the root value, or the value
 *                          of a key that is not the last one, is not an object: the reference's type errors).
 *                          *records = number of records; cap = room in index_out (records).
 *   sjhip_count_where_path number of records whose element at `path` exists and satisfies `op`:
 *                          EXISTS; EQ_STRING (value = vlen bytes, compared after unescaping, Iter.StringBytes);
 *                          EQ_INT / EQ_UINT / EQ_FLOAT (value = an int64_t / uint64_t / double, vlen 8; the element is
 *                          converted the way Iter.Int / Uint / Float convert between the three number tags,
 *                          parsed_json.go:560-727 -- with the amd64 results at the two edges the reference lets through:
 *                          a float of exactly 2^63 is MinInt64 for EQ_INT, one of exactly 2^64 is 0 for EQ_UINT); EQ_BOOL (value = one byte); IS_NULL.  8 bytes cross PCIe.
 *   sjhip_project_keys     Object.ForEach(fn, onlyKeys) (parsed_object.go:142-196) on the root object of every record: the
 *                          members whose key is in the set, in document order, at most n_keys of them (the reference stops
 *                          after len(onlyKeys) deliveries).  out[r * n_keys + j] = key number << 56 | tape index of the
 *                          value of the j-th delivered member, ~0 when there is no j-th.  The keys must be distinct. */
#define SJHIP_PATH_NOT_FOUND (~0ull)
#define SJHIP_PATH_NOT_OBJECT (~0ull - 1ull)
enum { SJHIP_OP_EXISTS = 0, SJHIP_OP_EQ_STRING = 1, SJHIP_OP_EQ_INT = 2, SJHIP_OP_EQ_UINT = 3, SJHIP_OP_EQ_FLOAT = 4,
       SJHIP_OP_EQ_BOOL = 5, SJHIP_OP_IS_NULL = 6,
       /* the ordering operators and the prefix test (the numbering is part of the ABI): see sjhip_where_path below */
       SJHIP_OP_LT_INT = 7, SJHIP_OP_LE_INT, SJHIP_OP_GT_INT, SJHIP_OP_GE_INT,
       SJHIP_OP_LT_UINT, SJHIP_OP_LE_UINT, SJHIP_OP_GT_UINT, SJHIP_OP_GE_UINT,
       SJHIP_OP_LT_FLOAT, SJHIP_OP_LE_FLOAT, SJHIP_OP_GT_FLOAT, SJHIP_OP_GE_FLOAT,
       SJHIP_OP_PREFIX_STRING /* = 19 */ };
int sjhip_find_path(sjhip_ctx *ctx, const uint8_t *keys, const uint32_t *key_lens, uint32_t n_keys, uint64_t *index_out,
                    size_t cap, size_t *records);
int sjhip_count_where_path(sjhip_ctx *ctx, const uint8_t *keys, const uint32_t *key_lens, uint32_t n_keys, int op,
                           const void *value, size_t vlen, uint64_t *count);
int sjhip_project_keys(sjhip_ctx *ctx, const uint8_t *keys, const uint32_t *key_lens, uint32_t n_keys, uint64_t *out,
                       size_t cap_records, size_t *records);
/* Columns: the VALUE at `path` of every record, converted on the device, so that only the column crosses PCIe (the
 * reference's Iter.FindElement(path...) followed by a conversion of the element; records, paths, the probe with too small
 * a cap_records (SJHIP_ERR_ARG, *records set) and the limits are those of sjhip_find_path):
 *   sjhip_extract_path     what Iter.Float / Int / Uint / Bool (parsed_json.go:560-749, 867-875) return: `values` holds
 *                          cap_records doubles / int64_t / uint64_t (FLOAT / INT / UINT) or bytes 0 / 1 (BOOL), `status`
 *                          one byte per record; a record whose status is not OK has the value 0.  The number conversions
 *                          are those of sjhip_count_where_path (the amd64 results at 2^63 for INT and 2^64 for UINT).
 *   sjhip_extract_path_strings  Iter.StringBytes (the unescaped string), or with SJHIP_COL_CVT Iter.StringCvt
 *                          (parsed_json.go:775-800: strings as they are, integers in decimal, floats as appendFloat writes
 *                          them -- the text of MarshalJSON --, true / false / null; objects and arrays are TYPE), built on
 *                          the device: *records, *bytes = the total length of the column.
 *   sjhip_fetch_path_strings    the column in Arrow's "large string" layout: offsets[records + 1] (offsets[0] = 0), data[bytes],
 *                          status[records]; a record that is not OK has an empty slot.  The column stays on the device
 *                          until the next parse or the next sjhip_extract_path_strings of the context (other queries,
 *                          MarshalJSON and the serializer leave it alone); without one: SJHIP_ERR_ARG. */
enum { SJHIP_COL_FLOAT = 0, SJHIP_COL_INT = 1, SJHIP_COL_UINT = 2, SJHIP_COL_BOOL = 3 };
enum { SJHIP_COL_OK = 0, SJHIP_COL_NOT_FOUND = 1, /* ErrPathNotFound */
       SJHIP_COL_NOT_OBJECT = 2,                  /* the root value, or that of a key that is not the last one, is not an object */
       SJHIP_COL_TYPE = 3,                        /* "unable to convert type ..." / "value is not string" / StringCvt of {} [] */
       SJHIP_COL_NULL = 4,                        /* the element is null and the conversion rejects it (a type error there) */
       SJHIP_COL_RANGE = 5 };                     /* overflows / underflows int64; negative or above 2^64 for UINT */
int sjhip_extract_path(sjhip_ctx *ctx, const uint8_t *keys, const uint32_t *key_lens, uint32_t n_keys, int kind, void *values,
                       uint8_t *status, size_t cap_records, size_t *records);
#define SJHIP_COL_CVT 1u /* StringCvt instead of StringBytes */
int sjhip_extract_path_strings(sjhip_ctx *ctx, const uint8_t *keys, const uint32_t *key_lens, uint32_t n_keys, uint32_t flags,
                               size_t *records, size_t *bytes);
int sjhip_fetch_path_strings(sjhip_ctx *ctx, uint64_t *offsets, uint8_t *data, uint8_t *status);
/* Aggregates: count, sum, min and max of the column sjhip_extract_path(path, kind) would return, reduced on the device -- the
 * reference's loop of Iter.FindElement(path...) and Iter.Float / Int / Uint over the records (or, under a row selection, over the
 * rows), with the additions and comparisons a caller writes behind it.  88 bytes cross PCIe instead of 9 per row.
 *   sjhip_aggregate_path          over all rows of the selection in force (without one: the root value of every record).
 *   sjhip_aggregate_path_records  one entry per RECORD: record r reduces the rows row_offsets[r] .. row_offsets[r + 1] that
 *                          sjhip_fetch_rows returns (without a selection: its one row, the root value).  A record without rows,
 *                          or without an OK row, has count 0, sum 0 (+0.0) and min = max = 0; the record's own status byte
 *                          (NOT_FOUND, TYPE, ...) is sjhip_fetch_rows' to tell.  Any destination may be NULL.  cap_records /
 *                          *records: the probe of sjhip_extract_path (too small a cap: SJHIP_ERR_ARG with *records set).
 * The element of a row, its conversion and its status byte are exactly sjhip_extract_path's (the amd64 results at 2^63 for INT
 * and at 2^64 for UINT included): kind = SJHIP_COL_FLOAT / INT / UINT; SJHIP_COL_BOOL, the string kinds and unknown kinds are
 * SJHIP_ERR_ARG and sjhip_last_error names the kind.  n_keys == 0 is allowed, as in sjhip_where_path: the element is the row's
 * own value (a selection of scalar rows, "prices":[1,2,3]).  Paths and limits are otherwise sjhip_find_path's.  Only the rows
 * whose status is SJHIP_COL_OK take part in sum, min and max; every row is counted in status[] / not_ok.
 *   sum    INT, UINT: exact, 128 bits, independent of the order of the rows.  FLOAT: IEEE double addition of the OK values in a
 *          fixed association that depends on the number of rows and on the selection's offsets only -- two calls on the same
 *          result return the same bits -- and that is NOT the document order: it is a tree over tiles of rows, and the parts of
 *          a sharded result are added in part order.  No floating-point atomics are used.
 *   min, max   INT, UINT: as integers.  FLOAT: the total order of the non-NaN doubles with -0.0 below +0.0 (the bit pattern
 *          with all bits of a negative value flipped and the sign bit of the others, compared as uint64_t), so the result does
 *          not depend on the order of the rows.  A tape the parser built holds no NaN and no Inf; for a deserialized tape that
 *          does, sum, min and max are whatever IEEE addition and that key order give.
 * Neither call creates, changes or drops a product or the selection, both work after parses with and without
 * SJHIP_FLAG_COPY_STRINGS and on sharded results (shards are cut at record boundaries: the per-record entries are laid end to
 * end in document order, the totals joined on the host).  No result on the device, a bad path, a bad kind: SJHIP_ERR_ARG,
 * sjhip_last_error has the reason and nothing was touched.  Without rows nothing is launched and the outputs are still filled. */
typedef struct sjhip_agg {
    uint64_t rows;            /* the rows looked at: *records of sjhip_find_path on the same selection */
    uint64_t status[6];       /* rows per SJHIP_COL_* status of the conversion; only status[SJHIP_COL_OK] rows take part below */
    uint64_t sum_lo, sum_hi;  /* FLOAT: sum_lo = the bits of the double, sum_hi = 0.  INT: the 128-bit two's-complement sum.
                                 UINT: the 128-bit unsigned sum.  (lo = low 64 bits) */
    uint64_t min, max;        /* bits of a double / an int64_t / a uint64_t; both 0 when no row is OK */
} sjhip_agg;                  /* 88 bytes: all that crosses PCIe */
int sjhip_aggregate_path(sjhip_ctx *ctx, const uint8_t *keys, const uint32_t *key_lens, uint32_t n_keys, int kind,
                         sjhip_agg *out);
int sjhip_aggregate_path_records(sjhip_ctx *ctx, const uint8_t *keys, const uint32_t *key_lens, uint32_t n_keys, int kind,
                                 uint64_t *count /* OK rows */, uint64_t *not_ok /* rows with any other status */,
                                 void *sum /* 8 B each: double, or the low 64 bits */, uint64_t *sum_hi,
                                 void *min, void *max, size_t cap_records, size_t *records);
/* Groups ("group by"): the distinct keys at a path as a dictionary in first-occurrence order, a code into it for every row, and the
 * aggregates above per distinct key -- the loop a caller of the reference writes with a map from Iter.StringBytes / Iter.Int to a
 * running count and sum, on the device.  The rows are those of the selection in force (without one: the root value of every
 * record), numbered in that order.
 *   key of a row   Iter.FindElement(key path) on the row, then key_kind = SJHIP_COL_STRING: Iter.StringBytes, the unescaped bytes
 *                  (the empty string is a key; "A" and its escaped spelling, backslash u0041, are one key, with and without SJHIP_FLAG_COPY_STRINGS), or
 *                  SJHIP_COL_INT: Iter.Int, exactly sjhip_extract_path's conversion (1, 1.0 and 1.9 are the key 1).  Every other
 *                  key kind is SJHIP_ERR_ARG.  key_n_keys == 0: the key is the row's own value ("hashtags":["a","b","a"]).
 *                  status[row] is the byte sjhip_extract_path[_strings] would give; a row whose status is not SJHIP_COL_OK is in
 *                  no group and has the code SJHIP_GROUP_NONE.
 *   groups         two OK rows are in one group iff their keys are equal (same length and bytes / same int64).  Group g's first
 *                  row comes before group g + 1's: codes, dictionary, first_row and group_rows are decided by the input alone.
 *   per group      first_row (the row number of its first row), group_rows (its rows), and with a value column the six arrays of
 *                  sjhip_aggregate_path_records with the group in the place of the record: the value of a row is
 *                  FindElement(value path) + the conversion of val_kind = SJHIP_COL_FLOAT / INT / UINT (val_n_keys == 0: the row's
 *                  own value); count = the group's rows whose value is OK, not_ok = the rest; sums, min and max as described above
 *                  (the float association depends on the rows and their grouping only; no floating-point atomics).
 *                  val_kind = SJHIP_GROUP_NO_VALUE: no value column is evaluated, val_keys / val_key_lens are ignored and may be
 *                  NULL, and sjhip_fetch_group_aggregates is SJHIP_ERR_ARG ("no value column").
 * sjhip_group_path builds the grouping on the device and returns its sizes: *rows, *groups and *key_bytes (STRING: the bytes of
 * all keys; INT: 8 * groups).  Without rows nothing is launched and all three are 0; rows without a single OK key: *groups = 0.
 *   sjhip_fetch_groups            key_offsets [groups + 1] and keys (key_bytes bytes end to end) for STRING keys -- Arrow's large
 *                                 string layout, key_offsets[0] = 0 is written even without groups --, or keys = int64_t[groups]
 *                                 for INT keys (key_offsets is ignored); first_row, group_rows [groups]; codes, status [rows].
 *   sjhip_fetch_group_aggregates  count, not_ok, sum, sum_hi, min, max [groups] each.
 * Any destination may be NULL.  (codes, keys) is the dictionary-encoded column an Arrow consumer takes in place of the strings.
 * Lifetime: the grouping is a product of its own with its own device arena (counted by sjhip_ctx_device_bytes, freed by
 * sjhip_ctx_trim); it lasts until the next parse or the next sjhip_group_path, is materialised data -- it survives a change or drop
 * of the selection and every other product, and they survive it -- and a call that fails behind its argument checks leaves no
 * grouping (as sjhip_extract_table leaves no table).  Each path has the limits of sjhip_find_path.
 * Errors: SJHIP_ERR_ARG, with sjhip_last_error naming the reason and nothing touched (the previous grouping included): no result on
 * the device, a bad path, an unknown key or value kind, a fetch without a grouping, and a sharded ND result ("... is sharded":
 * joining the dictionaries of shards is not done here).  More than 2^30 rows: SJHIP_ERR_TOOBIG. */
#define SJHIP_GROUP_NONE 0xffffffffu
#define SJHIP_GROUP_NO_VALUE (-1)
int sjhip_group_path(sjhip_ctx *ctx, const uint8_t *key_keys, const uint32_t *key_key_lens, uint32_t key_n_keys, int key_kind,
                     const uint8_t *val_keys, const uint32_t *val_key_lens, uint32_t val_n_keys, int val_kind,
                     size_t *rows, size_t *groups, size_t *key_bytes);
int sjhip_fetch_groups(sjhip_ctx *ctx, uint64_t *key_offsets, void *keys, uint64_t *first_row, uint64_t *group_rows,
                       uint32_t *codes, uint8_t *status);
int sjhip_fetch_group_aggregates(sjhip_ctx *ctx, uint64_t *count, uint64_t *not_ok, void *sum, uint64_t *sum_hi,
                                 void *min, void *max);
/* Groups by several keys: the distinct TUPLES of up to SJHIP_GROUP_MAX_KEYS key columns, and the aggregates of up to
 * SJHIP_GROUP_MAX_VALUES value columns per tuple, from one grouping ("tickets and total fine per (Make, Color)").  keys, key_lens
 * and the path lengths are laid out as in sjhip_extract_table and sjhip_order_paths: all paths end to end, the key columns first,
 * then the value columns; key_path_lens[c] / val_path_lens[v] keys each (0: the row's own value).  Each path has the limits of
 * sjhip_find_path; all paths together hold at most 32 keys and 1024 bytes.  n_key_cols is 1 to 8, n_val_cols 0 to 8 (0: val_path_lens
 * and val_kinds may be NULL).
 *   key_kinds[c]   SJHIP_COL_STRING (Iter.StringBytes: the unescaped bytes, with and without SJHIP_FLAG_COPY_STRINGS), SJHIP_COL_INT,
 *                  SJHIP_COL_UINT or SJHIP_COL_BOOL: sjhip_extract_path's conversion and status byte (1, 1.0 and 1.9 are the INT key
 *                  1).  SJHIP_COL_FLOAT, SJHIP_COL_STRING_CVT and everything else: SJHIP_ERR_ARG, naming the column and the kind.
 *   val_kinds[v]   SJHIP_COL_FLOAT, SJHIP_COL_INT or SJHIP_COL_UINT, as sjhip_group_path's value column.
 *   key_flags[c]   0 or SJHIP_GROUP_NULL_KEY; NULL: all 0; any other bit is SJHIP_ERR_ARG.
 *   tuple of a row one entry per key column: the converted key where the column's status is SJHIP_COL_OK.  Under
 *                  SJHIP_GROUP_NULL_KEY a row with any other status on that column (NOT_FOUND, NOT_OBJECT, NULL, TYPE, RANGE alike)
 *                  has the entry "no key" -- the rows without a key on a column tie with each other on it, as in
 *                  sjhip_order_paths --; without the flag such a row is in no group and has the code SJHIP_GROUP_NONE.
 *   groups         two rows are in one group iff their tuples are equal entry by entry: both "no key", or the same bytes / value.
 *                  Column boundaries count: ("ab","c") and ("a","bc") differ.  Groups are numbered by the first occurrence of
 *                  their tuple; codes, first_row and group_rows are as in sjhip_group_path and decided by the input alone.
 * sjhip_group_paths returns *rows, *groups and key_bytes[c] for every key column: STRING: the bytes of the column's entries over all
 * groups (one entry per group: a key that two groups share counts twice); INT, UINT: 8 * groups; BOOL: groups.
 *   sjhip_fetch_group_keys(col)          column col's entry of every group: key_offsets [groups + 1] and keys [key_bytes[col]] for
 *                                        STRING (key_offsets[0] = 0 is written even without groups); int64_t / uint64_t [groups] for
 *                                        INT / UINT, uint8_t [groups] for BOOL (key_offsets is ignored).  key_ok[g] = 1 where group
 *                                        g has a key on the column, 0 for "no key" (an empty string slot, or the value 0).
 *                                        status [rows]: every row's status byte on this column -- every row is evaluated on
 *                                        every key column, whatever the others give.
 *   sjhip_fetch_group_aggregates_at(val) the six arrays of sjhip_fetch_group_aggregates for value column val: rows, conversion, the
 *                                        tree association of float sums and the 128-bit integer sums are sjhip_group_path's.
 * Any destination may be NULL; a column the grouping does not have is SJHIP_ERR_ARG.
 * A context holds ONE grouping, built by either call, and each fetch works on it where it is unambiguous: sjhip_fetch_groups gives
 * first_row, group_rows and codes of any grouping, and key_offsets / keys / status of column 0 when there is exactly one key column
 * (with more, a non-NULL one is SJHIP_ERR_ARG naming sjhip_fetch_group_keys); sjhip_fetch_group_aggregates is value column 0 when
 * there is exactly one (else SJHIP_ERR_ARG: "no value column", or naming sjhip_fetch_group_aggregates_at); the two fetches here work
 * on a grouping of sjhip_group_path: column 0 (key_ok all 1) and value 0.  With one STRING or INT key column, flags 0 and at most one
 * value column the call IS sjhip_group_path, bit for bit through both families of fetches.
 * Everything else is sjhip_group_path's: the rows are those of the selection in force (it composes with sjhip_where_path,
 * sjhip_unnest_rows and sjhip_order_*), the arena, the lifetime and what survives what, no rows (nothing is launched, an empty
 * grouping with all sizes 0 is published), argument errors that touch nothing -- the previous grouping included --, a later failure
 * that leaves no grouping, 2^30 rows, and a sharded result refused.
 * Not done here: joining the groupings of sharded results; FLOAT keys; a further value column on an existing grouping without
 * grouping again; HAVING-style filtering of groups (a caller orders or filters the fetched aggregates). */
#define SJHIP_GROUP_MAX_KEYS 8
#define SJHIP_GROUP_MAX_VALUES 8
#define SJHIP_GROUP_NULL_KEY 1u /* per key column */
int sjhip_group_paths(sjhip_ctx *ctx, const uint8_t *keys, const uint32_t *key_lens, const uint32_t *key_path_lens,
                      const int *key_kinds, const uint32_t *key_flags, uint32_t n_key_cols, const uint32_t *val_path_lens,
                      const int *val_kinds, uint32_t n_val_cols, size_t *rows, size_t *groups, size_t *key_bytes /* [n_key_cols] */);
int sjhip_fetch_group_keys(sjhip_ctx *ctx, uint32_t col, uint64_t *key_offsets, void *keys, uint8_t *key_ok /* [groups] */,
                           uint8_t *status /* [rows] */);
int sjhip_fetch_group_aggregates_at(sjhip_ctx *ctx, uint32_t val, uint64_t *count, uint64_t *not_ok, void *sum, uint64_t *sum_hi,
                                    void *min, void *max);
/* List columns: the ARRAY at `path` of every record, converted on the device -- the reference's Iter.FindElement(path...),
 * Iter.Array() and then Array.AsFloat / AsInteger / AsUint64 / AsString / AsStringCvt (parsed_array.go:145-344); paths, records
 * and limits are those of sjhip_find_path.
 *   sjhip_extract_path_list          kind = SJHIP_COL_FLOAT / INT / UINT (SJHIP_COL_BOOL: SJHIP_ERR_ARG, the reference has no such
 *                          conversion); *records, *elems = the records and the elements of all their arrays together.
 *   sjhip_fetch_path_list            Arrow's large_list<T>: list_offsets[records + 1] (list_offsets[0] = 0; record r owns the elements
 *                          list_offsets[r] .. list_offsets[r + 1]), values[elems] (8 bytes each: double / int64_t / uint64_t),
 *                          status[records].
 *   sjhip_extract_path_list_strings  Array.AsString, or with SJHIP_COL_CVT Array.AsStringCvt; *bytes = the bytes of all the texts.
 *   sjhip_fetch_path_list_strings    Arrow's large_list<large_string>: list_offsets as above, str_offsets[elems + 1] (element e owns
 *                          data[str_offsets[e] .. str_offsets[e + 1]]), data[bytes], status[records].
 * A record whose status is not SJHIP_COL_OK has an empty slot, and so has an OK record whose array is empty: the status byte
 * tells the two apart.  The statuses are the SJHIP_COL_* values above:
 *   NOT_FOUND / NOT_OBJECT  from FindElement, as for the scalar columns;
 *   NULL                    the element at the path is null (the scalar columns' convention: a dataframe maps it to a null list);
 *   TYPE                    any other element at the path that is not an array (Iter.Array: "next item is not array");
 *   inside the array the reference returns at the first element it cannot convert: the record's status is that of the FIRST
 *   failing element in document order.
 *     AsFloat      l / u / d elements: float64(int64), float64(uint64), the double as it is; any other element -- null, strings,
 *                  true / false, nested containers -- is TYPE.
 *     AsInteger    a u element above MaxInt64, a d element > 2^63 or < -2^63: RANGE; a d element of exactly 2^63 is MinInt64 (the
 *                  amd64 result, as for the scalar column).
 *     AsUint64     an l or d element < 0: RANGE (-0.0 passes and gives 0); a d element > 2^63: RANGE; exactly 2^63 gives 1 << 63.
 *     AsString     every element must be a string (its unescaped bytes), else TYPE.
 *     AsStringCvt  every element converted like the scalar column's SJHIP_COL_CVT (numbers in decimal / as appendFloat writes them,
 *                  true / false / null); TYPE for a nested object or array.
 *   What differs from the scalar columns: a null ELEMENT is TYPE, not NULL (parsed_array.go has no case for it), for AsString too;
 *   AsUint64 rejects floats in (2^63, 2^64], which Iter.Uint converts (parsed_array.go:253 compares with math.MaxInt64, Iter.Uint with
 *   math.MaxUint64), and so never meets the 2^64 edge; there is no bool conversion.
 * The list column lives in a device arena of its own: it and the string column of sjhip_extract_path_strings survive each other,
 * the other queries, MarshalJSON and the serializer; it lasts until the next parse or the next list extraction of the context
 * (sjhip_ctx_device_bytes counts it, sjhip_ctx_trim frees it).  A fetch without a list column, or of the other kind (the numeric
 * fetch after a string extraction or the reverse), is SJHIP_ERR_ARG and sjhip_last_error says so.  On a sharded ND result every
 * shard builds its part and the fetch joins them. */
int sjhip_extract_path_list(sjhip_ctx *ctx, const uint8_t *keys, const uint32_t *key_lens, uint32_t n_keys, int kind, size_t *records,
                            size_t *elems);
int sjhip_fetch_path_list(sjhip_ctx *ctx, uint64_t *list_offsets, void *values, uint8_t *status);
int sjhip_extract_path_list_strings(sjhip_ctx *ctx, const uint8_t *keys, const uint32_t *key_lens, uint32_t n_keys, uint32_t flags,
                                    size_t *records, size_t *elems, size_t *bytes);
int sjhip_fetch_path_list_strings(sjhip_ctx *ctx, uint64_t *list_offsets, uint64_t *str_offsets, uint8_t *data, uint8_t *status);
/* Tables: columns at SEVERAL paths from ONE walk of every record.  The single-column calls above walk every record from its root
 * once per call, and the walk is what they cost; a table of n columns -- each a path and a kind -- is evaluated together: the
 * paths' keys form a trie, every member of a record is compared once with the keys that may follow where the walk stands, and
 * the values are converted on the device and kept there until they are fetched column by column.
 *   sjhip_extract_table       `keys` holds the keys of all paths end to end; column c owns the next path_lens[c] entries of
 *                          key_lens.  kinds[c] = SJHIP_COL_FLOAT / INT / UINT / BOOL, SJHIP_COL_STRING (Iter.StringBytes) or
 *                          SJHIP_COL_STRING_CVT (Iter.StringCvt).  *records = the records; bytes[c] = the text length of a string
 *                          column, 0 for a numeric or bool column.
 *   sjhip_fetch_table_column  a numeric or bool column: values[records] (8 bytes each, 1 byte for BOOL) and status[records];
 *                          offsets and data are ignored and may be NULL.  A string column: offsets[records + 1], data[bytes[col]]
 *                          and status[records]; values is ignored.
 * Column c is exactly what sjhip_extract_path(path c, kind c) returns, or sjhip_extract_path_strings(path c) followed by
 * sjhip_fetch_path_strings: the same values bit for bit, the same status bytes, offsets and bytes, the same conventions (value 0
 * where the status is not OK, an empty slot for a string record that is not OK, the amd64 results at 2^63 and 2^64).  FindElement's
 * rules hold for every column: into the root and into objects, not into arrays; the first member with the key wins at every level
 * and nothing is taken back -- if the first "a" is not an object, a.b is NOT_OBJECT even if a later "a" is one; if it is an object
 * without "b", a.b is NOT_FOUND.  Two columns may name the same path with different kinds, and one path may be the beginning of
 * another.  Limits: 1 to SJHIP_TABLE_MAX_COLS columns, 1 to 16 keys per path, at most 32 keys and 1024 bytes in all paths together;
 * beyond them, for an unknown kind and for an empty path: SJHIP_ERR_ARG, and sjhip_last_error names which.
 * The table lives in device arenas of its own: it survives the string column, the list column, the filter, the serializer,
 * MarshalJSON and the other queries, and they survive it; it lasts until the next parse or the next sjhip_extract_table of the
 * context (sjhip_ctx_device_bytes counts it, sjhip_ctx_trim frees it).  A fetch without a table, or of a column the table does not
 * have, is SJHIP_ERR_ARG and sjhip_last_error says which.  On a sharded ND result every shard builds its table and the fetch
 * joins the column (string offsets rebased by the bytes in front).  SJHIP_COL_STRING / _STRING_CVT are kinds of table columns
 * only: sjhip_extract_path and sjhip_extract_path_list refuse them. */
#define SJHIP_TABLE_MAX_COLS 16
enum { SJHIP_COL_STRING = 4, SJHIP_COL_STRING_CVT = 5 };
int sjhip_extract_table(sjhip_ctx *ctx, const uint8_t *keys, const uint32_t *key_lens, const uint32_t *path_lens, const int *kinds,
                        uint32_t n_cols, size_t *records, size_t *bytes /* [n_cols] */);
int sjhip_fetch_table_column(sjhip_ctx *ctx, uint32_t col, void *values, uint64_t *offsets, uint8_t *data, uint8_t *status);
/* Rows: the elements of the ARRAY at `path` of every record become the records of the path queries -- the reference's
 * Iter.FindElement(path...) -> Iter.Array() -> Array.Iter() / Advance over the elements (what {"statuses":[{...}, ...]}, a root array
 * of objects or an NDJSON line {"order":1,"items":[{...},{...}]} need before anything above can be pointed at their objects).
 *   sjhip_select_rows     evaluates FindElement + Iter.Array on the root value of every record, as the list columns do, with their
 *                          status bytes: OK, NOT_FOUND, NOT_OBJECT, NULL for a null element, TYPE for anything else that is not an
 *                          array.  The direct elements of that array, in document order, are the rows -- scalars, objects and arrays
 *                          alike; what lies inside an element is not a row.  A record whose status is not OK, or whose array is
 *                          empty, has no rows.  n_keys == 0 is allowed here, and only here: the array is then the record's root value
 *                          (keys and key_lens may be NULL).  Paths and limits are otherwise those of sjhip_find_path.  *records = the
 *                          records, *rows = the rows of all of them together; no rows at all is a legal selection.
 *   sjhip_fetch_rows      Arrow's list layout over the records: row_offsets[records + 1] (row_offsets[0] = 0; record r owns the rows
 *                          row_offsets[r] .. row_offsets[r + 1]), row_index[rows] = the tape index of the value of every row
 *                          (tape[index] is its tag word; in the merged index space on a sharded result), status[records].  Any
 *                          destination may be NULL: that array is not copied.
 *   sjhip_select_records  back to one row per record; no error if nothing was selected.
 * While a selection exists, the calls that evaluate a path on "every record" evaluate it on every ROW instead, the row's value in the
 * place of the record's root value: sjhip_find_path, sjhip_count_where_path, sjhip_project_keys, sjhip_extract_path,
 * sjhip_extract_path_strings, sjhip_extract_path_list[_strings] and sjhip_extract_table; their *records and cap_records count rows.
 * A row that is not an object gets SJHIP_PATH_NOT_OBJECT / SJHIP_COL_NOT_OBJECT, the rule for a root value that is not an object.
 * With no rows they return *records = 0 and launch nothing.  sjhip_count_where, sjhip_filter_where, the serializer, MarshalJSON and
 * the stream's filter work on records and ignore the selection (sjhip_filter_rows below is the filter that reads it).
 * The selection lives in a device arena of its own (sjhip_ctx_device_bytes counts it, sjhip_ctx_trim frees it): it lasts until the
 * next parse, the next sjhip_select_rows or sjhip_select_records, is dropped by everything that drops the other products, survives
 * the string column, the list column, the table, the filter, the serializer and MarshalJSON, and they survive it.  A column, list or
 * table built under a selection is materialised data: it stays fetchable after the selection has changed or gone.  sjhip_fetch_rows
 * without a selection is SJHIP_ERR_ARG and sjhip_last_error says "no row selection".  On a sharded ND result every shard selects its
 * rows (shards are cut at record boundaries: an array never spans two) and the fetch joins them.  The cost is a fixed number of
 * passes over the tape, whatever the arrays' lengths and whatever the elements hold. */
int sjhip_select_rows(sjhip_ctx *ctx, const uint8_t *keys, const uint32_t *key_lens, uint32_t n_keys, size_t *records, size_t *rows);
int sjhip_fetch_rows(sjhip_ctx *ctx, uint64_t *row_offsets /* [records + 1] */, uint64_t *row_index /* [rows] */,
                     uint8_t *status /* [records] */);
int sjhip_select_records(sjhip_ctx *ctx);
/* Row predicates: keep the rows whose element at `path` satisfies a test -- the WHERE of the columns, lists and tables above; what a
 * Go caller writes as FindElement(path...), the Iter conversion and a Go comparison, for every row at once.
 *   sjhip_where_path      The predicate is the one of sjhip_count_where_path: the element at `path` of the row EXISTS and satisfies
 *                          `op` -- the operators above, and
 *                            LT / LE / GT / GE _INT / _UINT / _FLOAT  (value = an int64_t / uint64_t / double, vlen 8) the element converted
 *                                      exactly as EQ_INT / EQ_UINT / EQ_FLOAT convert it -- Iter.Int / Uint / Float: a float is truncated
 *                                      for INT, with the amd64 results at 2^63 and 2^64 -- then compared as int64_t, uint64_t or double;
 *                                      an element whose conversion is not SJHIP_COL_OK (null, a type error, a range error)
 *                                      satisfies nothing;
 *                            PREFIX_STRING  the element is a string whose unescaped bytes (Iter.StringBytes) begin with the vlen
 *                                      bytes of `value` (at most the 1024 bytes EQ_STRING allows; vlen 0 matches every string).
 *                          sjhip_count_where_path accepts these operators too: its count is *rows of sjhip_where_path on the same
 *                          selection.  flags: SJHIP_WHERE_NOT keeps exactly the rows the same call without it drops -- the rows
 *                          where the path is not found, where an object is missing on the way and where the conversion fails
 *                          included; any other bit is SJHIP_ERR_ARG.  n_keys == 0 is allowed, as in sjhip_select_rows: the element
 *                          is the row's own value (a selection whose rows are scalars).  Paths and limits are otherwise those of
 *                          sjhip_find_path.
 * What it narrows: with a row selection in force, the selection keeps its records and their status bytes, and every record keeps
 * the matching ones among the rows it owned, in document order.  Without one it creates a selection in which record r owns one
 * row -- its root value -- if it matches and none otherwise, every status SJHIP_COL_OK.  Either way the result is an ordinary row
 * selection: sjhip_fetch_rows delivers it, sjhip_select_records and everything that drops a selection drop it, every call that
 * runs on rows runs on the kept rows, and successive calls are the conjunction of their predicates.  *records = the records,
 * *rows = the rows kept; keeping no rows is legal (the rules of a selection without rows above).  sjhip_count_where,
 * sjhip_filter_where, the stream's filter, the serializer and MarshalJSON keep ignoring the selection.
 * Failure: a call that fails with SJHIP_ERR_ARG -- an unknown operator or flag, a value of the wrong size or too long, a bad path,
 * no result on the device -- leaves the selection exactly as it was.  A call that fails later (SJHIP_ERR_HIP) gives the selection
 * up, as sjhip_select_records does, and sjhip_last_error says so.  On a sharded ND result every shard narrows its own rows and
 * the fetch joins them.  The cost is one walk of every row and a fixed number of passes over arrays of at most 8 bytes per row. */
#define SJHIP_WHERE_NOT 1u
int sjhip_where_path(sjhip_ctx *ctx, const uint8_t *keys, const uint32_t *key_lens, uint32_t n_keys, int op, const void *value,
                     size_t vlen, uint32_t flags, size_t *records, size_t *rows);
/* Row predicates of SEVERAL tests: up to 16 predicates evaluated in ONE walk of every row and combined with AND / OR / NOT -- a
 * disjunction ("Make is HOND or TOYT", "lang in (en, ja, es)"), which no sequence of sjhip_where_path calls can express, and a
 * conjunction or a range on one path without a walk, a compaction and a host wait per test.
 *   predicates  keys / key_lens / path_lens are laid out as in sjhip_extract_table: predicate p owns the next path_lens[p] entries
 *               of key_lens; path_lens[p] == 0: the row's own value.  The paths have the limits of a table (16 keys each, 32 keys
 *               and 1024 key bytes together; empty paths do not count).  ops[p] is any SJHIP_OP_* above.  `values` holds the
 *               values end to end and value_lens[p] is what sjhip_where_path takes for ops[p]: 8 for the numeric operators, 1 for
 *               EQ_BOOL, 0 for EXISTS and IS_NULL, 0 to 1024 for EQ_STRING / PREFIX_STRING; at most 1024 bytes together.
 *               Predicate p is TRUE for a row iff the element at its path exists and satisfies ops[p]: sjhip_where_path's
 *               predicate with flags 0.  FindElement's rules hold per path: the first member with the key wins.
 *   program     postfix, 1 to SJHIP_WHERE_MAX_PROGRAM bytes: a byte 0 .. n_preds - 1 pushes that predicate's truth,
 *               SJHIP_WHERE_AND and SJHIP_WHERE_OR pop two values and push one, SJHIP_WHERE_NEG replaces the top.  It must never
 *               underflow, end with exactly one value, name every predicate at least once and hold no other byte.  NEG over a
 *               predicate keeps exactly what SJHIP_WHERE_NOT keeps: the rows where the path is missing or the conversion fails
 *               included.  "a in (x, y)" is two predicates on one path and `0 1 OR`; a range is `0 1 AND`.
 *   sjhip_where_paths        narrows the selection exactly as sjhip_where_path does, for the predicate "the program is true": the
 *                            same composition with earlier and later calls, a selection is created when there is none, *records
 *                            and *rows, keeping no rows is legal, every shard of a sharded result narrows its own rows, a call that
 *                            fails with SJHIP_ERR_ARG leaves the selection as it was and a later failure gives it up.
 *   sjhip_count_where_paths  *count = *rows of that call, and the selection is not touched.
 * SJHIP_ERR_ARG, with sjhip_last_error naming the predicate or the program position: n_preds outside 1 .. 16, an unknown operator,
 * a value of the wrong size, paths beyond the limits of a table, an invalid program.  The cost is one walk of every row, whatever
 * n_preds is, and sjhip_where_path's passes behind it. */
#define SJHIP_WHERE_MAX_PREDS 16      /* = SJHIP_TABLE_MAX_COLS: one plan */
#define SJHIP_WHERE_MAX_PROGRAM 64
enum { SJHIP_WHERE_AND = 0x80, SJHIP_WHERE_OR = 0x81, SJHIP_WHERE_NEG = 0x82 };  /* program bytes; 0 .. 15 push predicate p */
int sjhip_where_paths(sjhip_ctx *ctx, const uint8_t *keys, const uint32_t *key_lens, const uint32_t *path_lens,
                      const int *ops, const void *values, const uint32_t *value_lens, uint32_t n_preds,
                      const uint8_t *program, uint32_t program_len, size_t *records, size_t *rows);
int sjhip_count_where_paths(sjhip_ctx *ctx, const uint8_t *keys, const uint32_t *key_lens, const uint32_t *path_lens,
                            const int *ops, const void *values, const uint32_t *value_lens, uint32_t n_preds,
                            const uint8_t *program, uint32_t program_len, uint64_t *count);
/* Row predicates by MEMBERSHIP: keep the rows whose key at `path` is one of a set of values -- the result of one query narrowing
 * another ("the tickets whose Make is one of the 200 makes sjhip_fetch_groups just returned", "the statuses whose user.id is in
 * this list of 50 000 ids", and with SJHIP_WHERE_NOT "the plugins whose name is not in the installed set"): a semi-join, and an
 * anti-join, whose cost per row does not depend on the size of the set.
 *   the set        kind = SJHIP_COL_STRING: value_offsets[n_values + 1] and `values` as bytes end to end -- Arrow's large-string layout,
 *                  exactly what sjhip_fetch_groups, sjhip_fetch_group_keys and sjhip_fetch_path_strings hand out; value_offsets[0] == 0
 *                  and the offsets never decrease.  kind = SJHIP_COL_INT: `values` is int64_t[n_values]; SJHIP_COL_UINT:
 *                  uint64_t[n_values]; value_offsets is ignored for both and may be NULL.  Every other kind (FLOAT, BOOL, STRING_CVT,
 *                  unknown) is SJHIP_ERR_ARG and sjhip_last_error names the kind.  Duplicates are legal and change nothing.
 *                  n_values == 0 is legal: no row matches, and all three pointers may be NULL.
 *   the predicate  a row matches iff the set holds a value s for which sjhip_where_path on the same path with SJHIP_OP_EQ_STRING /
 *                  EQ_INT / EQ_UINT and s, flags 0, would keep it: a string is compared by its unescaped bytes, with and without
 *                  SJHIP_FLAG_COPY_STRINGS; under INT the elements 1, 1.0 and 1.9 all match 1; an element that is missing, null, of
 *                  the wrong type or out of range matches nothing.  flags: SJHIP_WHERE_NOT keeps exactly the rows the same call
 *                  without it drops, the rows without a usable key included; any other bit is SJHIP_ERR_ARG.  n_keys == 0: the row's
 *                  own value.  Paths have the limits of sjhip_find_path.
 *   sjhip_where_path_in        narrows what sjhip_where_path narrows, as it narrows it: with a selection the records keep their
 *                  status bytes and the matching rows among those they owned; without one a selection is created, one row per
 *                  matching record; *records and *rows as there; it composes with every earlier and later where / order / unnest
 *                  call; keeping no rows is legal; the other products survive it.
 *   sjhip_count_where_path_in  *count = *rows of that call; nothing is touched.
 * SJHIP_ERR_ARG, with sjhip_last_error naming the reason, and nothing touched -- all checked on the host before anything is
 * uploaded or launched, the number of values before any of them is read: no result on the device, a bad path, a bad kind, unknown
 * flag bits, n_values > SJHIP_WHERE_IN_MAX_VALUES, a NULL `values` or `value_offsets` where one is needed, value_offsets[0] != 0 or an
 * offset smaller than the one in front (the index is named), a string value longer than the 1024 bytes EQ_STRING allows (the index
 * is named).  A call that fails later (SJHIP_ERR_HIP) gives the selection up, as sjhip_where_path does.  On a sharded ND result
 * every shard narrows its own rows (each builds the table for itself) and the fetch joins them.
 * The uploaded values, their hashes and the table over them -- the grouping's hash and open-addressing table, at most half full --
 * are working data of the call in a device arena of their own (sjhip_ctx_device_bytes counts it, sjhip_ctx_trim frees it): nothing
 * of them can be fetched and nothing refers to them afterwards.  The cost is sjhip_where_path's, plus the upload of the set and
 * one lane per value to build the table. */
#define SJHIP_WHERE_IN_MAX_VALUES (1u << 24)
int sjhip_where_path_in(sjhip_ctx *ctx, const uint8_t *keys, const uint32_t *key_lens, uint32_t n_keys, int kind,
                        const uint64_t *value_offsets, const void *values, size_t n_values, uint32_t flags,
                        size_t *records, size_t *rows);
int sjhip_count_where_path_in(sjhip_ctx *ctx, const uint8_t *keys, const uint32_t *key_lens, uint32_t n_keys, int kind,
                              const uint64_t *value_offsets, const void *values, size_t n_values, uint32_t flags,
                              uint64_t *count);
/* Order rows ("order by ... limit k"): rank the rows of the selection in force (without one: the root value of every record) by a
 * numeric key at a path and keep the first `limit` of them -- "the 10 most retweeted statuses" without the column, the host sort and
 * the rows that are thrown away crossing PCIe.
 *   key of a row   Iter.FindElement(path) on the row, converted by kind = SJHIP_COL_FLOAT / INT / UINT: exactly sjhip_extract_path's
 *                  value and status byte (the amd64 results at 2^63 and 2^64 included).  n_keys == 0: the row's own value.
 *                  SJHIP_COL_BOOL, the string kinds and unknown kinds are SJHIP_ERR_ARG and sjhip_last_error names the kind.
 *   order          the rows whose status is SJHIP_COL_OK first, ascending by key -- INT as int64_t, UINT as uint64_t, FLOAT in the
 *                  total order of the aggregates' min / max (-0.0 below +0.0) --, with SJHIP_ORDER_DESC descending; equal keys stay
 *                  in row order in both directions (the sort is stable; 0.0 and an integer 0 tie under FLOAT).  The rows whose
 *                  status is not OK come behind all OK rows, in row order, in both directions (NULLS LAST; a caller who does not
 *                  want them filters first).  The rank of a row is its position in that order.  Any other flag bit: SJHIP_ERR_ARG.
 *   limit          0, or at least the number of rows: every row is kept.  Otherwise the rows of rank < limit are kept; stability
 *                  decides which of a run of equal keys crosses the limit.
 * The call narrows the selection and builds a product.  The selection stays in document order: it is narrowed exactly as
 * sjhip_where_path would narrow it for the predicate "rank < limit" -- records keep the kept rows they owned and their status bytes,
 * without a selection one is created, successive sjhip_where_path and sjhip_order_path calls compose.  *records = the records,
 * *rows = the rows kept.  The order of the kept rows is a product of its own:
 *   sjhip_fetch_order   order[i] = the row number, IN THE SELECTION AS THIS CALL LEFT IT, of the row of rank i -- a permutation of
 *                       0 .. rows - 1 that the host applies with one take to what it fetches for the kept rows (text rows through
 *                       the offsets of sjhip_fetch_marshaled_rows); values[i] = that row's converted key (8 bytes each: a double,
 *                       an int64_t or a uint64_t; 0 where not OK), sorted, the rows without an OK key at its tail; status[i] = that
 *                       row's status byte.  Any destination may be NULL.  With limit = 0 this is a full ORDER BY.
 * Lifetime: the order has its own device arena (counted by sjhip_ctx_device_bytes, freed by sjhip_ctx_trim) and lasts until the
 * next parse or the next sjhip_order_path; it survives changes and drops of the selection and of every other product, and they
 * survive it -- but its row numbers refer to the selection as this call left it, not to a later one.  Works after parses with and
 * without SJHIP_FLAG_COPY_STRINGS.  Without rows nothing is launched, *rows = 0 and an empty order is published.
 * Errors: SJHIP_ERR_ARG, with sjhip_last_error naming the reason and nothing touched (the selection and the previous order stay as
 * they were): no result on the device, a bad path, a bad kind, unknown flag bits, a fetch without an order, and a sharded ND
 * result ("... is sharded": the ranks of shards are not merged here).  More than 2^30 rows: SJHIP_ERR_TOOBIG.  A call that fails
 * later (SJHIP_ERR_HIP) gives the selection up, as sjhip_where_path does, and leaves no order.  The cost is one walk of every row,
 * and one sort pass of 8 key bits for every byte position in which the keys differ at all (counts below 2^20: three, not eight). */
#define SJHIP_ORDER_DESC 1u
int sjhip_order_path(sjhip_ctx *ctx, const uint8_t *keys, const uint32_t *key_lens, uint32_t n_keys, int kind,
                     uint32_t flags, uint64_t limit, size_t *records, size_t *rows);
int sjhip_fetch_order(sjhip_ctx *ctx, uint64_t *order /* [rows] */, void *values /* [rows], 8 B each */, uint8_t *status /* [rows] */);
/* Order rows by a STRING key: sjhip_order_path for the keys JSON carries as text -- dates, ids, names.
 *   key of a row   Iter.FindElement(path) on the row, then Iter.StringBytes: the status byte is the one sjhip_extract_path_strings
 *                  gives without SJHIP_COL_CVT (OK for a string, else NOT_FOUND / NOT_OBJECT / NULL / TYPE), the key the UNESCAPED
 *                  bytes -- "A" and its escaped spelling are one key, after parses with and without SJHIP_FLAG_COPY_STRINGS.
 *                  n_keys == 0: the row's own value.
 *   order          the OK rows first, ascending by bytes.Compare: unsigned bytes from the left, a proper prefix in front of the
 *                  longer key.  The empty string is the smallest key, and a NUL byte (an escaped U+0000) is a byte like any other:
 *                  "a" < "a" NUL < "a" NUL NUL.  For valid UTF-8 this is the order of the code points; it is NOT a collation (no
 *                  locale, no case folding, no normalisation: "z" sorts in front of "e" with an acute accent).  SJHIP_ORDER_DESC: the
 *                  reverse order of the distinct keys.  Equal keys stay in row order and the rows without an OK key come last in
 *                  row order, in both directions; any other flag bit is SJHIP_ERR_ARG.
 * Everything else -- limit, the narrowing of the selection, *records / *rows, the composition with sjhip_where_path,
 * sjhip_unnest_rows and further order calls, "no rows launches nothing and publishes an empty order", the 2^30 rows, the refusal of
 * a sharded result and the failure rules -- is sjhip_order_path's, see there.  The product is the same one: a context holds ONE
 * order, numeric or string, and sjhip_fetch_order(order, NULL, status) delivers it.  A string order has no 8-byte values: a non-NULL
 * `values` is SJHIP_ERR_ARG.  The sorted keys are sjhip_extract_path_strings on the kept rows, taken through order[].
 * The cost is one walk of every row and, for every 7 key bytes that rows still tie on, one round over those rows: a sort pass
 * for every byte position that differs, and one wait of the host.  The rounds end with the longest key. */
int sjhip_order_path_strings(sjhip_ctx *ctx, const uint8_t *keys, const uint32_t *key_lens, uint32_t n_keys, uint32_t flags, uint64_t limit,
                             size_t *records, size_t *rows);
/* Order rows by SEVERAL keys: "tickets by Make, then by Fine descending", "statuses by user.screen_name, then newest first" -- the
 * order a stable sort by the tuple of up to SJHIP_ORDER_MAX_KEYS key columns gives, ties refined column by column on the device.
 *   keys, key_lens, path_lens   laid out as in sjhip_extract_table: the keys of all paths end to end, column c owns the next
 *                  path_lens[c] entries of key_lens.  path_lens[c] == 0: the key is the row's own value.  Each path has the limits of
 *                  sjhip_find_path; all paths together hold at most 32 keys and 1024 bytes.
 *   kinds[c]       SJHIP_COL_FLOAT / INT / UINT: key and status byte are sjhip_order_path's (the amd64 results at 2^63 and 2^64 and
 *                  the float total order with -0.0 below +0.0 included); SJHIP_COL_STRING: those of sjhip_order_path_strings (the
 *                  unescaped bytes, compared as bytes.Compare, in both copy modes).  Anything else is SJHIP_ERR_ARG and
 *                  sjhip_last_error names the column and the kind.
 *   flags[c]       SJHIP_ORDER_DESC per column; any other bit is SJHIP_ERR_ARG.  flags == NULL: all ascending.
 *   n_cols         1 to SJHIP_ORDER_MAX_KEYS.
 *   order          rows are compared on column 0: the rows whose status there is SJHIP_COL_OK first, ascending by key or, with
 *                  SJHIP_ORDER_DESC, in the reverse order of the distinct keys, the rows without an OK key behind them (NULLS LAST
 *                  in both directions).  Rows that tie on column 0 -- the rows without an OK key there tie with each other -- are
 *                  compared on column 1 in the same way, and so on: a column's rows without a key come last within their tie class,
 *                  not last overall.  Rows that tie on every column stay in row order.
 * With n_cols == 1 the call is sjhip_order_path or sjhip_order_path_strings, bit for bit: the same selection and the same order[].
 * Everything else -- limit (applied once, at the end), the narrowing of the selection, *records / *rows, the composition with
 * sjhip_where_path, sjhip_unnest_rows and further order calls, "no rows launches nothing and publishes an empty order", the 2^30
 * rows, the refusal of a sharded result, "argument errors touch nothing" and "a later failure gives the selection up and leaves no
 * order" -- is sjhip_order_path's, see there.  The product is the context's one order: sjhip_fetch_order(order, NULL, status)
 * delivers it, status[i] being the status byte ON COLUMN 0 of the row of rank i -- the only column every row is evaluated on.  It
 * has no 8-byte values: a non-NULL `values` is SJHIP_ERR_ARG.  The sorted keys are sjhip_extract_table on the kept rows, taken
 * through order[].
 * The cost is one walk of every row for column 0 and its rounds (a numeric column has one, a string column one per 7 key bytes that
 * rows still tie on); a column behind the first walks and sorts only the rows that still tie in front of it, and is skipped
 * when none does.  Every round is one wait of the host. */
#define SJHIP_ORDER_MAX_KEYS 8
int sjhip_order_paths(sjhip_ctx *ctx, const uint8_t *keys, const uint32_t *key_lens, const uint32_t *path_lens, const int *kinds,
                      const uint32_t *flags, uint32_t n_cols, uint64_t limit, size_t *records, size_t *rows);
/* Unnest rows: the elements of the ARRAY at `path` of every ROW become the rows -- a second Iter.FindElement(path...) -> Iter.Array()
 * -> Array.Iter() / Advance inside the loop over the outer elements: statuses[].entities.hashtags[], performances[].seatCategories[]
 * .areas[], items[].tags[].  Everything that runs on "the rows of the selection in force" then runs on the inner elements.
 *   sjhip_unnest_rows        evaluates FindElement + Iter.Array on the value of every row of the selection in force -- the PARENT rows;
 *                            without a selection they are the root values of the records -- with the status bytes sjhip_select_rows
 *                            gives a record: OK, NOT_FOUND, NOT_OBJECT (a scalar parent row with n_keys > 0 included), NULL, TYPE.
 *                            n_keys == 0 is allowed: the row's own value must be the array ([[1,2],[3]] -> sjhip_select_rows with no
 *                            keys -> sjhip_unnest_rows with no keys -> the rows 1, 2, 3).  Paths and limits are otherwise those of
 *                            sjhip_find_path.  The direct elements of those arrays, in document order, are the new rows -- scalars,
 *                            objects and arrays alike; what lies inside an element is not a row.  A parent whose status is not OK, or
 *                            whose array is empty, contributes none.
 *                            The selection is replaced by one over the same records: record r owns the new rows that came from the
 *                            rows it owned, in document order, and the status bytes of the records stay as they were (without a prior
 *                            selection: all OK, as when sjhip_where_path creates one).  The result is an ordinary selection:
 *                            sjhip_fetch_rows, every call that runs on rows, sjhip_where_path, sjhip_order_path, sjhip_group_path,
 *                            sjhip_aggregate_path[_records], sjhip_filter_rows, sjhip_marshal_rows and a further sjhip_unnest_rows work
 *                            on it unchanged.  *records = the records, *parents = the rows before the call, *rows = the rows after it.
 *                            No parents, or no rows, is legal: nothing is launched for a part without parents, and the (empty)
 *                            selection and an empty parents product are still published.
 *   sjhip_fetch_row_parents  the join back, Arrow's list layout over the parent rows: parent_offsets[parents + 1] (parent_offsets[0] = 0;
 *                            parent p produced the new rows parent_offsets[p] .. parent_offsets[p + 1]), parent[rows] = the parent row
 *                            number of every new row -- the array a host `take` needs to repeat a parent column, fetched before the
 *                            call, next to a child column --, parent_status[parents].  Any destination may be NULL.  Parent numbers
 *                            refer to THE SELECTION AS IT WAS BEFORE THE CALL, child numbers to THE SELECTION AS THE CALL LEFT IT, not to
 *                            a later one: after a later narrowing, match through row_index of sjhip_fetch_rows, which is stable -- the
 *                            tape index of a row's value does not change when rows around it are dropped.
 * Lifetime: the parents have their own device arena (counted by sjhip_ctx_device_bytes, freed by sjhip_ctx_trim) and last until the
 * next parse or the next sjhip_unnest_rows; they survive every change and drop of the selection and every other product, and they
 * survive them.  Works after parses with and without SJHIP_FLAG_COPY_STRINGS.  On a sharded ND result every shard unnests its own
 * rows and the fetch joins them: parent_offsets moved up by the rows in front, parent by the parents in front.
 * Errors: SJHIP_ERR_ARG, with sjhip_last_error naming the reason and nothing touched (the selection and the previous parents stay as
 * they were): a bad path, a null size pointer, no result on the device, a fetch without the product ("no row parents on the device
 * ...").  A call that fails later (SJHIP_ERR_HIP) gives the selection up, as sjhip_where_path does, leaves no parents and says so.
 * The cost is one walk of every parent row to its array and a fixed number of passes over the tape, whatever the arrays' lengths
 * and whatever the elements hold. */
int sjhip_unnest_rows(sjhip_ctx *ctx, const uint8_t *keys, const uint32_t *key_lens, uint32_t n_keys, size_t *records, size_t *parents,
                      size_t *rows);
int sjhip_fetch_row_parents(sjhip_ctx *ctx, uint64_t *parent_offsets /* [parents + 1] */, uint64_t *parent /* [rows] */,
                            uint8_t *parent_status /* [parents] */);
/* Member rows: the members of the OBJECT at `path` of every row become the rows -- Iter.FindElement(path...) -> Iter.Object() ->
 * Object.ForEach / NextElementBytes (parsed_object.go), the other half of sjhip_unnest_rows: JSON often keeps a collection as a map
 * from id to record ("events": {"138586341": {...}, ...}, "plugins": {"git": {...}, ...}).
 *   sjhip_unnest_members   sjhip_unnest_rows' contract with Iter.Object in the place of Iter.Array: the parents are the rows of the
 *                          selection in force (without one: the root values of the records); n_keys == 0: the row's own value must be
 *                          the object.  Parent status: OK, NOT_FOUND, NOT_OBJECT, NULL for a null target, TYPE for an array or a
 *                          scalar.  The new rows are the VALUES of the direct members, in document order; duplicate names each give
 *                          a row, as Object.ForEach visits them (not Object.Map's "the last one wins"); what lies inside a value is
 *                          not a row; an empty object, or a parent whose status is not OK, gives none.  Records keep their status
 *                          bytes and own what came from the rows they owned; the parents product is the one of sjhip_unnest_rows,
 *                          and sjhip_fetch_row_parents serves both calls.  The result is an ordinary selection: sjhip_fetch_rows,
 *                          every call that runs on rows, sjhip_where_path[s], sjhip_order_*, sjhip_group_*, sjhip_aggregate_*,
 *                          sjhip_filter_rows, sjhip_marshal_rows[_paths] and a further sjhip_unnest_rows / sjhip_unnest_members run
 *                          on it unchanged (a marshaled or filtered member is its value only).  Errors, failures, lifetime and
 *                          sharded ND results are those of sjhip_unnest_rows.
 *   sjhip_extract_row_names  the unescaped names of the rows in force (NextElementBytes' `name`) as the string column: the product of
 *                          sjhip_extract_path_strings, which it replaces, fetched by sjhip_fetch_path_strings as offsets[rows + 1],
 *                          data and status; every status is OK.
 *   sjhip_where_row_names  sjhip_where_path's narrowing with the row's name in the place of the element at a path ("the event whose
 *                          id is 138586341", "the plugins whose name begins with git").  op: SJHIP_OP_EQ_STRING or
 *                          SJHIP_OP_PREFIX_STRING, flags: SJHIP_WHERE_NOT; the limits on `value` are sjhip_where_path's.  Every
 *                          other operator: SJHIP_ERR_ARG.
 * The two name calls need the selection in force to be one of members -- the one sjhip_unnest_members left, or what sjhip_where_*,
 * sjhip_where_row_names and the limit of sjhip_order_* narrowed it to: the name of a row is read from the two tape words in front
 * of its value, nothing is stored per row.  After sjhip_select_rows, sjhip_unnest_rows, sjhip_select_records or a parse they
 * return SJHIP_ERR_ARG, touch nothing and say "the rows in force are not object members (sjhip_extract_row_names follows
 * sjhip_unnest_members)".  They work with and without SJHIP_FLAG_COPY_STRINGS and on sharded ND results.
 * The cost of sjhip_unnest_members is that of sjhip_unnest_rows: one walk of every parent to its object and a fixed number of
 * passes over the tape, whatever the objects' sizes. */
int sjhip_unnest_members(sjhip_ctx *ctx, const uint8_t *keys, const uint32_t *key_lens, uint32_t n_keys, size_t *records, size_t *parents,
                         size_t *rows);
int sjhip_extract_row_names(sjhip_ctx *ctx, size_t *records, size_t *bytes);
int sjhip_where_row_names(sjhip_ctx *ctx, int op, const void *value, size_t vlen, uint32_t flags, size_t *records, size_t *rows);
/* Row schema: which member names the rows in force have, how often each occurs and with values of which types -- what Arrow's JSON
 * reader or json_normalize find out before they build a table, without the tape crossing to the host.
 *   sjhip_row_schema        evaluates FindElement + Iter.Object on the value of every row of the selection in force (without one: the
 *                           root value of every record), with sjhip_unnest_members' status bytes; n_keys == 0: the row's own value
 *                           must be the object.  status[s] = the rows with status byte s (SJHIP_COL_OK .. SJHIP_COL_RANGE), *rows
 *                           their sum.  Every OK row contributes its direct members as Object.ForEach visits them -- a name that
 *                           occurs twice in one object counts twice --, *members is their number.  A name is the unescaped bytes
 *                           of the key ("\u0061" and "a" are one name, "a" and "A" are two, the empty name is a name); names are
 *                           numbered by first occurrence in document order, *names of them, *name_bytes in their dictionary.
 *   sjhip_fetch_row_schema  name_offsets[names + 1] and name_data[name_bytes]: the dictionary; first_row[k]: the number, in the
 *                           selection in force at the call, of the first row that has name k; counts[k * SJHIP_SCHEMA_TYPES + (T - 1)]:
 *                           the members named k whose value has type T -- the reference's Type of the value's tape tag (TagToType):
 *                           true and false are both BOOL; an integer that fits int64 is INT, a larger one UINT, anything with a
 *                           fraction or an exponent FLOAT.  The counts add up to *members.  Any destination may be NULL.
 * The call reads the selection and leaves it -- its rows, its `members` property, its depth --, the row parents and every other
 * product exactly as they were: sjhip_fetch_rows returns after it what it returned before.  The schema is a product of its own with
 * its own device arenas (counted by sjhip_ctx_device_bytes, freed by sjhip_ctx_trim) and lasts until the next parse or the next
 * sjhip_row_schema.  No rows, or no members, is legal: an empty schema is published and nothing more is launched than it takes to
 * know that.  Works after parses with and without SJHIP_FLAG_COPY_STRINGS.  Nested objects are not descended into: call again with
 * the path of a name whose OBJECT count is not zero.
 * Errors: SJHIP_ERR_ARG, with sjhip_last_error naming the reason and nothing touched (the previous schema included): no result on
 * the device, a bad path, a null size pointer, a fetch without a schema, a sharded ND result ("... is sharded": the dictionaries of
 * shards are not joined, as for the groups).  More than 2^28 members: SJHIP_ERR_TOOBIG -- known only after the members have been
 * counted, so, like a call that fails later (SJHIP_ERR_HIP), it leaves no schema (the previous one is gone) and the selection as
 * it was.  The cost is sjhip_unnest_members' walk and a fixed number of passes over the
 * members, whatever the number of distinct names. */
enum { SJHIP_TYPE_NULL = 1, SJHIP_TYPE_STRING = 2, SJHIP_TYPE_INT = 3, SJHIP_TYPE_UINT = 4, SJHIP_TYPE_FLOAT = 5,
       SJHIP_TYPE_BOOL = 6, SJHIP_TYPE_OBJECT = 7, SJHIP_TYPE_ARRAY = 8 };   /* the reference's Type values (TagToType) */
#define SJHIP_SCHEMA_TYPES 8
int sjhip_row_schema(sjhip_ctx *ctx, const uint8_t *keys, const uint32_t *key_lens, uint32_t n_keys,
                     size_t *rows, uint64_t status[6], uint64_t *members, size_t *names, size_t *name_bytes);
int sjhip_fetch_row_schema(sjhip_ctx *ctx, uint64_t *name_offsets /* [names + 1] */, uint8_t *name_data /* [name_bytes] */,
                           uint64_t *first_row /* [names] */, uint64_t *counts /* [names * SJHIP_SCHEMA_TYPES] */);
/* Filter rows: the rows of the selection in force -- sjhip_select_rows' or the one sjhip_where_path narrowed or created -- as a new
 * self-contained (Tape, Strings.B) on the device, one root per row: what a caller of ParseND reads with Iter.  With it,
 * sjhip_where_path followed by sjhip_filter_rows is sjhip_filter_where for every operator, for conjunctions and negation, for
 * nested paths and for rows inside arrays; only the wanted rows cross PCIe.
 *   sjhip_filter_rows     Every selected row whose value is an object or an array contributes, in selection order, an opening root
 *                          word 'r' << 56 | index behind its closing root, the row's tape words [v, payload(tape[v])), and a closing
 *                          root word 'r' << 56 | index of its opening root.  Inside the row the payload of every { } [ ] word is moved
 *                          by (new index - old index) and the payload of every string word to the new Strings.B; the second words of
 *                          strings and numbers are copied as they are.  The new Strings.B is the rows' string bytes end to end: a row
 *                          owns the bytes from its first string to the end of its last one (keys and the strings of nested containers
 *                          included).  The result is bit for bit the (Tape, Strings.B) ParseND with copied strings returns for the
 *                          document whose lines are the texts of those rows.  A selected row that is a scalar -- a string, a number,
 *                          true / false / null -- has no such tape (a scalar line is no document): it is left out and counted.
 *                          *n_rows = the rows emitted, *skipped = the scalar rows left out, *tape_len / *strings_len = the sizes of
 *                          the result; any of them may be NULL.  No row emitted is legal: both sizes are 0.  sjhip_fetch_filtered
 *                          copies the result to the host.
 * Errors: SJHIP_ERR_ARG, with sjhip_last_error naming the reason and nothing touched, without a whole result on the context (a sharded
 * ND result says so, as for sjhip_filter_where), without a row selection ("no row selection") and after a parse without
 * SJHIP_FLAG_COPY_STRINGS; SJHIP_ERR_TOOBIG if the result would exceed 2^32 - 1 tape words (every row gains two root words: the
 * result of [[],[],[]] is larger than its source).
 * The result is the filtered result of the context, like sjhip_filter_where's: it replaces the last filtered, serialized or marshaled
 * product and is replaced by the next one and by the next parse.  The selection, the string column, the list column and the table
 * stay as they are.  The cost is one pass over the words of the selected rows to measure them, a fixed number of passes over 16
 * bytes per row, and one pass that copies. */
int sjhip_filter_rows(sjhip_ctx *ctx, uint64_t *n_rows, uint64_t *skipped, size_t *tape_len, size_t *strings_len);

/* ---- Serializer.Serialize on the device (parsed_serialize.go:200-431, format version 3) -----------------------------
 * Splits the device-resident tape of the last parse (SJHIP_FLAG_COPY_STRINGS) into the reference's three columns --
 * tags (one byte per tape entry), values (8 / 16 bytes per value-bearing entry), strings (= Strings.B, the reference's
 * string buffer without de-duplication hits) -- and frames them as a CompressNone stream (every block type 0), which
 * the reference's Deserialize reads; S2 / zstd compression of the columns (CompressFast / Default / Best) is host work.
 *   serialize        : builds the columns on the device; sizes of the columns and of the framed stream
 *   fetch_serialized : writes the framed stream into `dst` (>= stream_len bytes): header varints from the host, the
 *                      three columns straight from the device */
int sjhip_serialize(sjhip_ctx *ctx, size_t *tags_len, size_t *values_len, size_t *strings_len, size_t *stream_len);
/* SJHIP_SER_DEDUP: strings are de-duplicated like the reference's indexString (parsed_serialize.go:836-857) does -- a
 * string equal to the first string of the document in its hash slot is stored once (2^20 slots; deterministic, where the
 * reference's table is keyed by a per-process random hash) -- and the string column holds the kept strings only. */
#define SJHIP_SER_DEDUP 1u
int sjhip_serialize_ex(sjhip_ctx *ctx, uint32_t flags, size_t *tags_len, size_t *values_len, size_t *strings_len,
                       size_t *stream_len);
int sjhip_fetch_serialized(sjhip_ctx *ctx, uint8_t *dst, size_t cap, size_t *len);
/* Serializer.Deserialize (parsed_serialize.go:466-695) of a stream whose blocks are uncompressed (what
 * sjhip_fetch_serialized writes; S2 / zstd blocks are decompressed on the host first): the tape is rebuilt on the device
 * from the tag and value columns (two prefix sums and one scatter pass; closing brackets from their openers).  Like the
 * reference's result the strings point into pj.Message (= the string column) and Strings.B is what the stream carried
 * (empty for version 3).  sjhip_fetch copies Tape / Strings.B, sjhip_fetch_message pj.Message (message_len bytes). */
int sjhip_deserialize(sjhip_ctx *ctx, const uint8_t *stream, size_t len, size_t *tape_len, size_t *strings_len,
                      size_t *message_len);
int sjhip_fetch_message(sjhip_ctx *ctx, uint8_t *dst);

/* ---- Iter.MarshalJSON on the device (parsed_json.go:401-556) ---------------------------------------------------------
 * The device-resident result of the last parse as compact JSON text, records separated by '\n' -- byte for byte what
 * pj.Iter().MarshalJSON() returns: escapeBytes for strings, strconv.AppendInt / AppendUint, appendFloat (the reference's
 * copy of Go's Ryu shortest formatting with its ES6-style %f / %e choice).  The text stays on the device until
 * sjhip_fetch_marshaled copies it into `dst` (>= text_len bytes).  SJHIP_ERR_TOOBIG for a document of 4 GiB or more that was
 * parsed without SJHIP_FLAG_COPY_STRINGS (the strings that are not copied then lie at message offsets beyond 32 bits). */
int sjhip_marshal_json(sjhip_ctx *ctx, size_t *text_len);
int sjhip_fetch_marshaled(sjhip_ctx *ctx, uint8_t *dst);
/* Marshal rows: the rows of the selection in force (sjhip_select_rows / sjhip_where_path) as NDJSON text, built on the device --
 * the last step of "read, keep the rows that match, write them back": only the text of the kept rows crosses PCIe.
 *   sjhip_marshal_rows          The compact JSON text of every selected row, in selection order, joined by '\n' (none behind the
 *                               last).  A row's text follows the per-entry rules of sjhip_marshal_json exactly: brackets as they
 *                               are, '"' + escapeBytes + '"' for strings, ':' behind a key, ',' behind a completed value unless a
 *                               closing bracket follows, strconv.AppendInt / AppendUint / appendFloat, true / false / null.  Unlike
 *                               sjhip_filter_rows a scalar row is not skipped: its text is the scalar's own ("a\"b", -3, 1e+21,
 *                               null), what Iter.MarshalJSON returns on a scalar element.  *n_rows = the rows written, *text_len =
 *                               the bytes; either may be NULL.  No rows is legal: text_len is 0.
 *   sjhip_fetch_marshaled_rows  The text (`text`, >= text_len bytes) and Arrow-style row offsets (`offsets`, n_rows + 1 entries):
 *                               offsets[i] = the first byte of row i, offsets[n_rows] = text_len + 1 -- as if the last row had its
 *                               newline too -- so that row i is text[offsets[i] .. offsets[i + 1] - 1) for every i.  Without rows
 *                               offsets[0] = 0.  Either destination may be NULL.  SJHIP_ERR_ARG after sjhip_marshal_json, whose text
 *                               has no rows.
 * The text is the marshaled product of the context, the same tenant as sjhip_marshal_json's: sjhip_fetch_marshaled copies it as
 * well, it replaces and is replaced by the filtered / serialized / marshaled products and the next parse; the row offsets live
 * behind the text with the text's lifetime.  The selection, the string column, the list column and the table stay as they are.
 * With SJHIP_FLAG_KEY_FLAGS on the parse the kernels read the parser's key flags; without it the call builds the same array once,
 * in a work array of its own (the text is the same either way).  Parses without SJHIP_FLAG_COPY_STRINGS are supported as in
 * sjhip_marshal_json, with the same SJHIP_ERR_TOOBIG rule for documents of 4 GiB or more.
 * Errors: SJHIP_ERR_ARG, with sjhip_last_error naming the reason and nothing touched, without a result on the device, without a row
 * selection ("no row selection") and on a sharded ND result (it says so, as sjhip_filter_rows does); a float that is INF or NaN
 * gives the error of sjhip_marshal_json ("INF or NaN number found").
 * The cost is one pass over the words and strings of the selected rows to measure them, a fixed number of passes over 8 bytes per
 * row, and one pass that writes. */
int sjhip_marshal_rows(sjhip_ctx *ctx, uint64_t *n_rows, size_t *text_len);
int sjhip_fetch_marshaled_rows(sjhip_ctx *ctx, uint64_t *offsets /* [n_rows + 1] */, uint8_t *text /* [text_len] */);
/* Project rows: sjhip_marshal_rows with a select list -- of every row of the selection in force only the elements at n_cols paths, as
 * one JSON object per row: {"id":1,"user":{...},"n":null}.
 *   paths    keys / key_lens / path_lens as in sjhip_extract_table and sjhip_where_paths: column c owns the next path_lens[c] entries
 *            of key_lens; path_lens[c] == 0 is the row's own value (sjhip_where_paths).  A table's limits: 1 to
 *            SJHIP_TABLE_MAX_COLS columns, at most 16 keys per path, 32 keys and 1024 key bytes in all paths together.  FindElement's
 *            rules hold per path as documented for tables: the first member with the key wins and nothing is taken back; two columns
 *            may name one path, one path may be the beginning of another.
 *   names    the member names of the output, end to end, name_lens[c] bytes each: empty, repeated, any bytes; at most 1024 bytes
 *            together.  NULL: every column is named by the last key of its path (an empty path is then SJHIP_ERR_ARG).
 *   a row    '{' + the present columns in column order, joined by ',' + '}'; a present column is '"' + escapeBytes(name) + '":' +
 *            the text of the element, byte for byte what sjhip_marshal_rows writes for a row whose value is that element (scalars,
 *            strings, objects, arrays).  A column is absent when its path gives SJHIP_PATH_NOT_FOUND or SJHIP_PATH_NOT_OBJECT (a
 *            scalar row: every column with keys): it is left out with its ',', or written as "name":null under SJHIP_PROJECT_NULLS.
 *            An element that is present and null is written as null either way.  A row with nothing present is {}.
 * Rows, *n_rows, *text_len, the joining '\n' and the fetch are sjhip_marshal_rows': the result is the marshaled product of the
 * context with the row offsets behind it, delivered by sjhip_fetch_marshaled_rows and sjhip_fetch_marshaled.  The selection, the
 * string column, the list column and the table stay as they are (the cell indexes live in the shared work arena, not in the
 * table's).  Key flags, parses without SJHIP_FLAG_COPY_STRINGS, SJHIP_ERR_TOOBIG and the INF / NaN error are sjhip_marshal_rows'.
 * Errors: SJHIP_ERR_ARG, with sjhip_last_error naming the column or the reason and nothing touched: no result on the device, no row
 * selection ("no row selection"), a sharded ND result, an unknown flag bit, n_cols outside 1..16, paths or names beyond the limits, a
 * NULL `names` with an empty path.
 * The cost is one walk of every row's members up to the last wanted one (sjhip_extract_table's), 8 bytes per cell written and read
 * twice, and sjhip_marshal_rows' passes over the words and strings of the cells alone. */
#define SJHIP_PROJECT_NULLS 1u /* an absent field is written as null instead of being left out */
int sjhip_marshal_rows_paths(sjhip_ctx *ctx, const uint8_t *keys, const uint32_t *key_lens, const uint32_t *path_lens,
                             uint32_t n_cols, const uint8_t *names, const uint32_t *name_lens, uint32_t flags,
                             uint64_t *n_rows, size_t *text_len);

/* ---- ParseNDStream: replaces the block pipeline of simdjson_amd64.go:101-216 --------------------------------------
 * The binding cuts the input into blocks that end at a record boundary (simdjson_amd64.go:155-176; tmpSize = 10 MiB)
 * and feeds them to a stream; every block is parsed as an independent NDJSON document with every string copied
 * (:180) and the results come back in submission order.  A stream owns `slots` blocks in flight, spread round robin
 * over `n_devices` devices starting at `first_device` (0 devices = all that are visible; 0 slots = 3 per device);
 * every slot has its own context, HIP stream, pinned input block and pinned result buffers, so the H2D copy of one
 * block, the kernels of another and the D2H copy of a third overlap.
 *   acquire  : a pinned block of sjhip_stream_block_capacity() bytes to read the input into (the reference's tmpPool);
 *              SJHIP_STREAM_FULL when every slot is busy (take a result first)
 *   grow     : a record that runs past the acquired block: a larger pinned block, the first `keep` bytes kept
 *   submit   : queue the acquired block (its first `len` bytes)            submit_copy = acquire + memcpy + submit
 *   next     : the result of the oldest outstanding block (blocks until it is done).  Tape / Strings.B / Message
 *              point into memory of the stream and stay valid until sjhip_stream_release (copy them into the
 *              caller's slices: the reference's `reuse` recycling is the caller's side of that copy).  A block that
 *              fails returns its error code (SJHIP_ERR_STAGE1 / _STAGE2 / ...), which ends the stream like the
 *              reference's first Stream{Error}: later calls return SJHIP_ERR_STREAM_CLOSED.  SJHIP_STREAM_EMPTY when
 *              nothing is outstanding (the caller reports io.EOF once its reader is exhausted).
 *   ready    : 1 if the oldest outstanding block has finished, i.e. sjhip_stream_next would return at once, else 0
 *              (a single-threaded caller drains finished blocks with it before every blocking read of its input,
 *              so that results are not withheld while the reader waits for more data)
 * The states, call by call (SJHIP_ERR_ARG leaves the stream exactly as it was):
 *   acquire  : with a block already acquired SJHIP_ERR_ARG, and that block stays the acquired one.  Slots are used in
 *              ring order: after cancel the same slot's block comes again.  *capacity is the slot's own, which is
 *              larger than sjhip_stream_block_capacity() (always what create was asked for) once the slot has grown.
 *   grow     : only with a block acquired (else SJHIP_ERR_ARG).  A new_capacity no larger than the slot's returns the
 *              same block.  The grown block stays with its slot for the life of the stream.
 *   submit   : without an acquired block, or with len beyond the slot's capacity, SJHIP_ERR_ARG; in the second case the
 *              block stays acquired (submit again with a valid len, grow, or cancel).  len = 0 is a block like any
 *              other: an empty document, i.e. SJHIP_ERR_STAGE1 when its turn comes.
 *   cancel, release : SJHIP_ERR_ARG without an acquired block / a held result.
 *   next     : while a result is held (not yet released) SJHIP_ERR_ARG, *out zeroed, the held result untouched; ready
 *              is 0 then, and the held block's slot counts as busy for acquire.  in_flight counts the blocks
 *              submitted and not yet handed out by next.
 *   closed   : after next has returned a block's error, next and acquire (so submit_copy) return
 *              SJHIP_ERR_STREAM_CLOSED; the first such next waits for the blocks still in flight and drops them
 *              (in_flight is 0 afterwards), and ready is 1: next does not wait.  Of several failing blocks in flight the
 *              one submitted first is reported, whichever finishes first, after every result in front of it.
 *   destroy  : at any time from the caller's thread(s) once no other call is running: queued blocks are dropped, a
 *              running one is waited for, a held result is given up.
 * One thread may submit while another takes results. */
typedef struct sjhip_stream sjhip_stream;
typedef struct sjhip_stream_result {
    const uint64_t *tape;
    size_t tape_len;
    const uint8_t *strings;
    size_t strings_len;
    const uint8_t *message; /* TrimSpace'd block (inside the pinned input block) */
    size_t message_len;
    int device;
    uint64_t records;       /* filtered streams (sjhip_stream_set_filter): matching records of the block, else 0 */
} sjhip_stream_result;
sjhip_stream *sjhip_stream_create(int first_device, int n_devices, size_t block_bytes, int slots, uint32_t flags);
void sjhip_stream_destroy(sjhip_stream *s);
size_t sjhip_stream_block_capacity(const sjhip_stream *s);
int sjhip_stream_slots(const sjhip_stream *s);
int sjhip_stream_in_flight(sjhip_stream *s);
const char *sjhip_stream_last_error(const sjhip_stream *s);
int sjhip_stream_acquire(sjhip_stream *s, uint8_t **block, size_t *capacity);
int sjhip_stream_grow(sjhip_stream *s, size_t keep, size_t new_capacity, uint8_t **block);
int sjhip_stream_submit(sjhip_stream *s, size_t len);
int sjhip_stream_cancel(sjhip_stream *s); /* hand the acquired block back unused */
int sjhip_stream_submit_copy(sjhip_stream *s, const uint8_t *block, size_t len);
int sjhip_stream_next(sjhip_stream *s, sjhip_stream_result *out);
int sjhip_stream_ready(sjhip_stream *s);
/* Compose the stream with sjhip_filter_where: every block is parsed and filtered on the device and only the matching
 * records' (Tape, Strings.B) -- identical to ParseND of the block's matching lines -- cross PCIe; result.records counts
 * them (a block without matches delivers the empty result: tape_len 0, strings_len 0).  Set before the first block is
 * submitted, or later while no block is acquired or in flight (else SJHIP_ERR_ARG, and the stream goes on as it was);
 * klen = 0 turns the filter off: results are whole blocks again and records is 0. */
int sjhip_stream_set_filter(sjhip_stream *s, const uint8_t *key, size_t klen, const uint8_t *value, size_t vlen);
int sjhip_stream_release(sjhip_stream *s);

/* ---- stage 1 only: replaces findStructuralIndices (stage1_find_marks_amd64.go:41-148) --------
 * pos_out receives ABSOLUTE uint32 byte positions (running sum of the reference's deltas).
 * *ok = the reference's return value (error_mask == 0 && indexTotal > 0 && end-of-doc checks). */
int sjhip_stage1(sjhip_ctx *ctx, const uint8_t *msg, size_t len, int ndjson, uint32_t *pos_out,
                 size_t pos_cap, size_t *n, int *ok);
/* device-resident variant: d_pos must hold pos_cap uint32; nothing is copied back but the counts */
int sjhip_stage1_device(sjhip_ctx *ctx, const void *d_msg, size_t len, int ndjson, void *d_pos,
                        size_t pos_cap, size_t *n, int *ok);
/* Queued form of sjhip_stage1_device for a caller that keeps several messages (or blocks of a stream) in flight, as
 * ParseNDStream's reader does with its 10 MB blocks (simdjson_amd64.go:127-215: the next block is read and indexed while the
 * previous one is parsed): _queue goes behind what is already on the context's stream and returns at once; the message
 * leaves count, end state and error bits in record `slot` (0 .. SJHIP_STAGE1_QUEUE_SLOTS-1) of the context's pinned host
 * memory.  Queued messages of one mode (ndjson or not) are grouped: several of them run as ONE launch of the kernel, so a
 * queued message starts when its group is full, when another call puts work on the context, and no later than the next
 * _wait -- not necessarily inside _queue.  _wait launches what is still queued and synchronises with the stream (a caller
 * that synchronises the stream itself must call _wait first); _result turns a record into (*n, *ok) exactly like
 * sjhip_stage1_device and must only be called for a slot whose message a _wait has covered (else SJHIP_ERR_HIP "left no
 * result").  A slot is free again once its result has been taken.  d_msg / d_pos of a queued message must stay untouched
 * until then; every message has its own verdict, count and positions, whatever it shares a launch with.
 * Because the launch is deferred, stream order no longer places a queued message in front of work the caller itself puts
 * on the context's stream (sjhip_ctx_set_stream) between _queue and _wait: a kernel of the caller's that reads d_pos, or
 * one that overwrites d_msg, must go behind _wait, not merely behind _queue.
 * If a group cannot be launched (a HIP error), all its messages are dropped: the call that tried to launch it -- _wait, or
 * a _queue whose message completed or displaced the group, in which case that message is not queued either -- returns the
 * error, and _result of every dropped message says "left no result".  The caller queues them again. */
#define SJHIP_STAGE1_QUEUE_SLOTS 64
int sjhip_stage1_device_queue(sjhip_ctx *ctx, const void *d_msg, size_t len, int ndjson, void *d_pos,
                              size_t pos_cap, int slot);
int sjhip_stage1_device_wait(sjhip_ctx *ctx);
int sjhip_stage1_device_result(sjhip_ctx *ctx, int slot, size_t len, size_t *n, int *ok);
/* launches the stage-1 kernel `iters` times back to back on the context's stream and returns the
 * average kernel duration in milliseconds measured with hipEvents on that stream */
int sjhip_stage1_time(sjhip_ctx *ctx, const void *d_msg, size_t len, int ndjson, void *d_pos,
                      size_t pos_cap, int iters, float *ms_per_launch);

/* ---- profiling aids (not needed by a binding) -------------------------------------------------------------------
 * sjhip_stage1_set_variant: kernel variant used by this process for stage 1 (A/B runs on hardware): 0 512-thread
 *   blocks with barriers, 1 1024 with barriers (default), 2 768 with barriers, 3 1024 barrier-free with 2 tiles in
 *   flight per block, 4 the same with 3, 5 1024 with barriers and one
 *   64-byte pass per lane instead of two (64 KiB tiles);
 *   -1 = the SJHIP_S1_VARIANT environment variable or the default.  Returns the variant in effect.  It applies to
 *   stage 1 alone (sjhip_stage1*, sjhip_stage1_trace); the whole parse always runs the default variant.
 * sjhip_stage1_trace: one stage-1 launch of a profiling build of the current variant that stamps s_memtime at the
 *   phase boundaries of every (tile, wave): trace_out[(tile * waves + wave) * words + k], k = 0 phase A begins,
 *   1 phase A done, 2 serial section done (only the wave that ran it), 3 state of the tile known, 4 flatten done,
 *   5 HW_ID | XCC_ID << 32.  Plain (non-ND) stage 1 of a device-resident message. */
int sjhip_stage1_set_variant(int variant);
/* The library can be built with -DSJ_DEBUG_BOUNDS (csrc/sj_bounds.h; __graft_entry__.build_lib(debug_bounds=True) ->
 * libsjhip_dbg.so): every array of the parse path is then reached through a bounds-checked view, and a parse during
 * which a kernel touched an element outside its array fails with SJHIP_ERR_HIP ("bounds check: ...").
 * sjhip_debug_bounds_selftest: -1 in the product build; in the debug build it runs a kernel with two deliberate
 * violations and returns how many were recorded (2). */
int sjhip_debug_bounds_selftest(void);
int sjhip_stage1_trace(sjhip_ctx *ctx, const void *d_msg, size_t len, void *d_pos, size_t pos_cap, uint64_t *trace_out,
                       size_t trace_cap_words, unsigned *tiles, int *waves, int *words);

/* ---- per-routine known-answer entry points (one 64-byte chunk, executed on the GPU) ----------
 * Same signatures as the Go wrappers in find_subroutines_amd64.go so that the reference's
 * per-routine tests (find_subroutines_amd64_test.go) can be replayed against the device code. */
int sjhip_find_odd_backslash_sequences(sjhip_ctx *ctx, const uint8_t in[64],
                                       uint64_t *prev_iter_ends_odd_backslash, uint64_t *odd_ends);      /* :86  */
int sjhip_find_quote_mask_and_bits(sjhip_ctx *ctx, const uint8_t in[64], uint64_t odd_ends,
                                   uint64_t *prev_iter_inside_quote, uint64_t *quote_bits,
                                   uint64_t *error_mask, uint64_t *quote_mask);                          /* :60  */
int sjhip_find_whitespace_and_structurals(sjhip_ctx *ctx, const uint8_t in[64], uint64_t *whitespace,
                                          uint64_t *structurals);                                        /* :206 */
int sjhip_finalize_structurals(sjhip_ctx *ctx, uint64_t structurals, uint64_t whitespace,
                               uint64_t quote_mask, uint64_t quote_bits,
                               uint64_t *prev_iter_ends_pseudo_pred, uint64_t *out);                     /* :35  */
int sjhip_find_newline_delimiters(sjhip_ctx *ctx, const uint8_t in[64], uint64_t quote_mask,
                                  uint64_t *mask);                                                       /* :40  */
int sjhip_flatten_bits_incremental(sjhip_ctx *ctx, uint32_t *base, int *base_index, uint64_t mask,
                                   uint64_t *carried, uint64_t *position);                               /* :229 */

#ifdef __cplusplus
}
#endif
#endif
