// sj_result.h -- what a context knows about the device-resident result of its last parse and the products derived from it.
// Plain C++ (no HIP): host_selftest.cpp replays the transitions on the CPU (tests/test_result_state.py).
//
// Three facts, each written only by the transitions below (the host files call them and ask the predicates):
//   * what the last parse left: nothing, a parse between its two phases, a whole result, one shard of a sharded ParseND (its stored
//     indices carry the three bases), or "my shards hold it" (an ND message beyond one context's reach, multi_api.hip parse_nd_big);
//     beside it, whether the key flags in d_keyflag belong to it and whether h_pack mirrors it;
//   * the tenant of the shared arenas d_q / d_qtape / d_qstrings: the filtered result, the serialized columns or the MarshalJSON text
//     -- one value, so at most one of them is resident;
//   * the string column (d_col), the list column (d_list, numbers or strings) and the table (d_table, d_tabledata), independent of
//     each other and of the tenant: one mechanism (Product) used three times -- and a fourth time for the row selection (d_rows:
//     "the rows are the elements of the array at this path"), which the path queries and the other three products are built over
//     while it exists and which they survive: what was built under a selection is materialised data.  The grouping (d_group:
//     sjhip_group_path) is the fifth use: built over the rows in force, independent of everything else once it exists.  The
//     order (d_order: sjhip_order_path) is the sixth: the rank order of the rows the call kept, materialised like the grouping.
//     The row parents (d_parents: sjhip_unnest_rows) are the seventh: which row of the selection the call found every row of the
//     selection it left came from, materialised like the other two.  The row schema (d_schema: sjhip_row_schema) is the eighth:
//     the distinct member names of the rows in force and their counts per value type, materialised; it reads the selection and
//     leaves it, and every other product, as they are.
// The rule: a parse call, successful or not, drops the previous result and everything derived from it (begin_parse); so do
// sjhip_deserialize, sjhip_ctx_trim and the stage-1-only calls (drop_result).  A product exists from its publish to the next
// transition that drops it; a product is only published on a resident result, and a result of no tape words is no result.
// Every context keeps its own state: the owner of a sharded result holds `sharded`, the joined sizes and the "exists" bits, each
// shard context holds its own part.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace sj {

class ResultState {
public:
    enum class Tenant : uint8_t { None, Filtered, Serialized, Marshaled };
    struct Filtered { size_t tape_len = 0, strings_len = 0; };
    struct Serialized { size_t tags = 0, vals = 0, slen = 0, rest = 0, stream = 0; bool dedup = false; };  // column sizes, framed stream
    struct Column { size_t records = 0, bytes = 0; };
    struct ListColumn { size_t records = 0, elems = 0, bytes = 0; bool strings = false; };  // (numbers or strings: what was published)
    static constexpr int TABLE_COLS = 16;  // SJHIP_TABLE_MAX_COLS
    // the records the selection ran over, the rows it found, and the depth of every row's value below its record's root value (0:
    // the rows are root values; sjhip_select_rows and every sjhip_unnest_rows / sjhip_unnest_members add n_keys + 1; a narrowing hands
    // it on); members: the rows are the values of object members (sjhip_unnest_members) -- the name of row r is the string two words
    // in front of its value; a narrowing hands it on, sjhip_select_rows and sjhip_unnest_rows publish it false
    struct Rows { size_t records = 0, rows = 0; uint32_t depth = 0; bool members = false; };
    struct Parents { size_t parents = 0, rows = 0; };  // the rows sjhip_unnest_rows ran over, the rows it left
    // the grouping (sjhip_group_path, sjhip_group_paths): the rows it ran over, its groups, and what its fetches need to know: the
    // kinds of its key columns (at least one in a published grouping; sjhip_group_path: exactly one) and of its value columns
    // (none: no aggregates were built), and the bytes of every key column's entries
    static constexpr int GROUP_COLS = 8;  // SJHIP_GROUP_MAX_KEYS, SJHIP_GROUP_MAX_VALUES
    struct Groups {
        size_t rows = 0, groups = 0;
        uint32_t key_cols = 0, val_cols = 0;
        int key_kinds[GROUP_COLS] = {}, val_kinds[GROUP_COLS] = {};
        size_t col_bytes[GROUP_COLS] = {};
    };
    // the order (sjhip_order_path): the rows it kept -- its arrays have that many entries -- and the kind of their keys
    struct Order { size_t rows = 0; int kind = 0; };
    // the row schema (sjhip_row_schema): the rows it ran over, the members it met, its distinct names and the bytes of their dictionary
    struct Schema { size_t rows = 0, members = 0, names = 0, name_bytes = 0; };
    struct Table {  // what a fetch of one column needs: its kind, and the text bytes of a string column (0 for the other kinds)
        size_t records = 0;
        uint32_t n_cols = 0;
        uint8_t kind[TABLE_COLS] = {};
        size_t bytes[TABLE_COLS] = {};
    };

    // ---- transitions ----
    // Every parse entry point, first: nothing of the last result is left.  (The sizes stay: they mean something under their flag only.)
    void begin_parse() {
        parse_ = Parse::None;
        key_flags_ = packed_ = false;
        tenant_ = Tenant::None;
        drop_products();
    }
    void drop_result() { begin_parse(); }  // the arenas of the result are re-used, freed or overwritten by something that is no parse
    void parse_pending() {  // phase 1 of a parse is queued
        begin_parse();
        parse_ = Parse::Pending;
    }
    // Phase 2 succeeded.  A result whose stored indices carry no bases is a whole one (the first shard of a sharded parse as well);
    // `packed`: the last launch also left it in h_pack (whole results only)
    void parse_done(uint64_t tape_base, uint64_t strings_base, uint64_t msg_base, size_t tape_len, bool key_flags, bool packed) {
        begin_parse();
        if (tape_len == 0) return;
        const bool whole = tape_base == 0 && strings_base == 0 && msg_base == 0;
        parse_ = whole ? Parse::Whole : Parse::Shard;
        tape_base_ = tape_base;
        strings_base_ = strings_base;
        msg_base_ = msg_base;
        key_flags_ = key_flags;
        packed_ = packed && whole;
    }
    void parse_sharded(size_t tape_len) {  // the shard contexts of this one hold the result
        begin_parse();
        if (tape_len) parse_ = Parse::Sharded;
    }
    // The shared arenas: a call gives up its own product before its checks (release_shared), claims the arenas before its first
    // write (the previous tenant is gone, whatever happens next) and publishes on success.  A publish without a result to publish
    // on changes nothing and says so: the caller made a mistake (sj_ctx.h published()).
    void release_shared(Tenant t) {
        if (tenant_ == t) tenant_ = Tenant::None;
    }
    void claim_shared() { tenant_ = Tenant::None; }
    bool publish_filtered(const Filtered &f) {
        if (!whole()) return false;
        tenant_ = Tenant::Filtered;
        filtered_ = f;
        return true;
    }
    bool publish_serialized(const Serialized &s) {
        if (!whole()) return false;
        tenant_ = Tenant::Serialized;
        serialized_ = s;
        return true;
    }
    bool publish_marshaled(size_t text_len) {  // (an owner: the joined length of its shards' texts)
        if (!resident() && !sharded()) return false;
        tenant_ = Tenant::Marshaled;
        marshaled_len_ = text_len;
        marshaled_by_rows_ = false;
        return true;
    }
    bool publish_marshaled_rows(size_t text_len, size_t rows) {  // the text of the selected rows: row offsets lie behind it
        if (!whole()) return false;
        tenant_ = Tenant::Marshaled;
        marshaled_len_ = text_len;
        marshaled_by_rows_ = true;
        marshaled_rows_ = rows;
        return true;
    }
    // The independent products: a call gives up the last one before anything can fail (begin) and publishes on success, on a
    // resident or sharded result only (an owner: the joined sizes of its shards' parts); sizes() mean something while exists().
    template <typename S>
    class Product {
        friend class ResultState;  // (publish)
        bool exists_ = false;
        S sizes_;

    public:
        void begin() { exists_ = false; }
        bool exists() const { return exists_; }
        const S &sizes() const { return sizes_; }
    };
    Product<Column> column;
    Product<ListColumn> list;
    Product<Table> table;
    Product<Rows> rows;  // the row selection (sjhip_select_rows; sjhip_select_records is its begin())
    Product<Groups> groups;  // the grouping (sjhip_group_path, sjhip_group_paths; d_group): materialised, independent of the selection it was built under
    Product<Order> order;    // the order (sjhip_order_path, d_order): materialised, its row numbers are those of the selection the call left
    // the row parents (sjhip_unnest_rows, d_parents): materialised; parent numbers are those of the selection the call found, row
    // numbers those of the selection it left
    Product<Parents> parents;
    // the row schema (sjhip_row_schema, d_schema): materialised; first_row counts in the selection the call ran under
    Product<Schema> schema;
    void publish_schema(const Schema &z) { (void)publish(&ResultState::schema, z); }  // (what sjhip_row_schema ends with)
    void drop_schema() { schema.begin(); }  // (... and what it begins with behind its argument checks)
    void drop_products() { column.begin(), list.begin(), table.begin(), rows.begin(), groups.begin(), order.begin(), parents.begin(), schema.begin(); }  // (a stage-1-only call on a sharded result: api.hip)
    template <typename S>
    bool publish(Product<S> ResultState::*product, const S &sizes) {  // publish(&ResultState::column, {records, bytes})
        if (!resident() && !sharded()) return false;
        (this->*product).exists_ = true;
        (this->*product).sizes_ = sizes;
        return true;
    }

    // ---- predicates ----
    bool pending() const { return parse_ == Parse::Pending; }
    bool whole() const { return parse_ == Parse::Whole; }                        // filter / serializer work on these
    bool resident() const { return whole() || parse_ == Parse::Shard; }          // path / count queries, MarshalJSON: a shard as well
    bool sharded() const { return parse_ == Parse::Sharded; }
    bool key_flags() const { return key_flags_; }
    bool packed() const { return packed_; }
    bool filtered() const { return tenant_ == Tenant::Filtered; }
    bool serialized() const { return tenant_ == Tenant::Serialized; }
    bool marshaled() const { return tenant_ == Tenant::Marshaled; }
    bool list_of(bool strings) const { return list.exists() && list.sizes().strings == strings; }  // a list column of this kind
    bool member_rows() const { return rows.exists() && rows.sizes().members; }  // the selection in force is one of object members

    // ---- what the last publish / parse_done left (meaningful while the predicate beside it holds) ----
    uint64_t tape_base() const { return tape_base_; }
    uint64_t strings_base() const { return strings_base_; }
    uint64_t msg_base() const { return msg_base_; }
    const Filtered &filtered_sizes() const { return filtered_; }
    const Serialized &serialized_sizes() const { return serialized_; }
    size_t marshaled_len() const { return marshaled_len_; }
    bool marshaled_by_rows() const { return marshaled() && marshaled_by_rows_; }  // sjhip_marshal_rows' text, not sjhip_marshal_json's
    size_t marshaled_rows() const { return marshaled_rows_; }

private:
    enum class Parse : uint8_t { None, Pending, Whole, Shard, Sharded };
    Parse parse_ = Parse::None;
    bool key_flags_ = false, packed_ = false;
    Tenant tenant_ = Tenant::None;
    uint64_t tape_base_ = 0, strings_base_ = 0, msg_base_ = 0;
    Filtered filtered_;
    Serialized serialized_;
    size_t marshaled_len_ = 0, marshaled_rows_ = 0;
    bool marshaled_by_rows_ = false;
};

}  // namespace sj
