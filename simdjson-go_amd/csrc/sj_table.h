// sj_table.h -- the plan of a table (sjhip_extract_table): n columns, each a path and a kind, evaluated in ONE walk per record.
// Plain C++ (no HIP): host_selftest.cpp exports the builder (sj_selftest_table_plan, tests/test_table_walk.py).
//
// The paths' keys form a trie: equal prefixes share a node, so a member of a record is compared once with the keys that may
// follow where the walk stands, however many columns pass through them.  The trie is flattened breadth first -- a parent in front
// of its children, the children of a node next to each other, in the order the columns named them -- into at most 32 nodes, one
// bit each in the walk's "matched" mask (sj_tablewalk.h).  The root of a record is no node: its children are nodes [0, root_n).
// The plan travels as a kernel argument; the keys travel in QView::key, node after node, as the keys of a path do.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace sj {

static constexpr int TABLE_MAX_COLS = 16;    // SJHIP_TABLE_MAX_COLS
static constexpr int TABLE_MAX_PATH = 16;    // keys of one path (QPATH_MAX)
static constexpr int TABLE_MAX_KEYS = 32;    // keys of all paths together = the most nodes a trie can have
static constexpr int TABLE_MAX_BYTES = 1024; // bytes of all keys together (QMAX)
static constexpr int TABLE_KINDS = 6;        // SJHIP_COL_FLOAT / INT / UINT / BOOL, SJHIP_COL_STRING, SJHIP_COL_STRING_CVT
static constexpr uint8_t TABLE_ROOT = 0xff;  // the parent of the root's children

struct TablePlan {
    uint16_t key_end[TABLE_MAX_KEYS];  // the key of node j = key[key_end[j - 1] .. key_end[j])
    uint16_t cols[TABLE_MAX_KEYS];     // the columns that end at node j (bit c)
    uint32_t sub[TABLE_MAX_KEYS];      // the nodes below node j (bit k): NOT_OBJECT together when its value is no object
    uint8_t parent[TABLE_MAX_KEYS];
    uint8_t child_b[TABLE_MAX_KEYS], child_n[TABLE_MAX_KEYS];  // its children: nodes [child_b, child_b + child_n)
    uint8_t kind[TABLE_MAX_COLS];
    uint32_t n_nodes, root_n, n_cols;
};

// why a table was refused (the text for sjhip_last_error: table_plan_error)
enum TablePlanError { TABLE_OK = 0, TABLE_ERR_COLS, TABLE_ERR_KIND, TABLE_ERR_EMPTY_PATH, TABLE_ERR_PATH_KEYS, TABLE_ERR_KEYS, TABLE_ERR_BYTES };
inline const char *table_plan_error(int e) {
    switch (e) {
    case TABLE_ERR_COLS: return "a table holds 1 to 16 columns";
    case TABLE_ERR_KIND: return "unknown column kind (SJHIP_COL_FLOAT / INT / UINT / BOOL / STRING / STRING_CVT)";
    case TABLE_ERR_EMPTY_PATH: return "a column's path holds no key";
    case TABLE_ERR_PATH_KEYS: return "a column's path holds more than 16 keys";
    case TABLE_ERR_KEYS: return "the paths of a table hold more than 32 keys together";
    case TABLE_ERR_BYTES: return "the keys of a table are longer than 1024 bytes together";
    }
    return "";
}

// keys: the keys of all paths end to end; column c owns the next path_lens[c] entries of key_lens.  -> TABLE_OK with the plan and
// the nodes' keys in blob[0 .. *blob_len) (node after node), or what is wrong; *bad_col: the column it was found at.
inline int table_plan(const uint8_t *keys, const uint32_t *key_lens, const uint32_t *path_lens, const int *kinds, uint32_t n_cols,
                      TablePlan *pl, uint8_t *blob /* [TABLE_MAX_BYTES] */, uint32_t *blob_len, uint32_t *bad_col) {
    *bad_col = 0;
    if (n_cols == 0 || n_cols > (uint32_t)TABLE_MAX_COLS) return TABLE_ERR_COLS;
    size_t n_keys = 0, n_bytes = 0;
    for (uint32_t c = 0; c < n_cols; c++) {
        *bad_col = c;
        if (kinds[c] < 0 || kinds[c] >= TABLE_KINDS) return TABLE_ERR_KIND;
        if (path_lens[c] == 0) return TABLE_ERR_EMPTY_PATH;
        if (path_lens[c] > (uint32_t)TABLE_MAX_PATH) return TABLE_ERR_PATH_KEYS;
        if (n_keys + path_lens[c] > (size_t)TABLE_MAX_KEYS) return TABLE_ERR_KEYS;
        for (uint32_t j = 0; j < path_lens[c]; j++) {
            n_bytes += key_lens[n_keys + j];
            if (n_bytes > (size_t)TABLE_MAX_BYTES) return TABLE_ERR_BYTES;
        }
        n_keys += path_lens[c];
    }
    // the trie, in the order the columns name its nodes
    struct Tmp {
        const uint8_t *key;
        uint32_t len;
        int parent;  // -1: the root
        uint16_t cols;
    } tmp[TABLE_MAX_KEYS];
    int nt = 0;
    size_t k = 0, at = 0;
    for (uint32_t c = 0; c < n_cols; c++) {
        int cur = -1;
        for (uint32_t j = 0; j < path_lens[c]; j++, k++) {
            const uint8_t *key = keys + at;
            const uint32_t len = key_lens[k];
            at += len;
            int hit = -1;
            for (int t = 0; t < nt && hit < 0; t++)
                if (tmp[t].parent == cur && tmp[t].len == len && (len == 0 || memcmp(tmp[t].key, key, len) == 0)) hit = t;
            if (hit < 0) {
                hit = nt++;
                tmp[hit] = {key, len, cur, 0};
            }
            cur = hit;
        }
        tmp[cur].cols |= (uint16_t)(1u << c);
    }
    // breadth first: order[q] = the trie node that becomes node q
    int order[TABLE_MAX_KEYS], newid[TABLE_MAX_KEYS], n = 0;
    for (int t = 0; t < nt; t++)
        if (tmp[t].parent < 0) order[n++] = t;
    memset(pl, 0, sizeof *pl);
    pl->root_n = (uint32_t)n;
    for (int q = 0; q < n; q++) {
        const int t = order[q];
        newid[t] = q;
        pl->child_b[q] = (uint8_t)n;
        for (int u = 0; u < nt; u++)
            if (tmp[u].parent == t) order[n++] = u;
        pl->child_n[q] = (uint8_t)(n - pl->child_b[q]);
    }
    uint32_t end = 0;
    for (int q = 0; q < n; q++) {
        const Tmp &t = tmp[order[q]];
        if (t.len) memcpy(blob + end, t.key, t.len);
        end += t.len;
        pl->key_end[q] = (uint16_t)end;
        pl->cols[q] = t.cols;
        pl->parent[q] = t.parent < 0 ? TABLE_ROOT : (uint8_t)newid[t.parent];
    }
    for (int q = n; q < TABLE_MAX_KEYS; q++) pl->key_end[q] = (uint16_t)end;
    for (int q = n - 1; q >= 0; q--)
        if (pl->parent[q] != TABLE_ROOT) pl->sub[pl->parent[q]] |= pl->sub[q] | (1u << q);
    for (uint32_t c = 0; c < n_cols; c++) pl->kind[c] = (uint8_t)kinds[c];
    pl->n_nodes = (uint32_t)n;
    pl->n_cols = n_cols;
    *blob_len = end;
    return TABLE_OK;
}

}  // namespace sj
