"""The plan and the walk of a table (csrc/sj_table.h, csrc/sj_tablewalk.h: sjhip_extract_table), restated on (Tape, Strings.B,
Message) arrays -- the checker of the C++ the kernel runs (sj_selftest_table_plan / sj_selftest_table_walk) and, per column, of
the device tables (test infrastructure, like column_walk.py, which pins it: tests/test_table_walk.py).

  plan    the trie of the paths' keys -- equal prefixes share a node --, flattened breadth first: a parent in front of its children,
          the children of a node next to each other, in the order the columns name them; the root of a record is no node
  walk    one pass over the members of a record: the first member that matches a not-yet-matched child of the current node marks
          it for good; a matched child with children is entered at once when its value is an object and takes everything below
          it to NOT_OBJECT when it is not
  table   walk + column_walk.convert / text per column, shaped like column_walk.column / string_column"""
import column_walk as CW
from query_walk import MASK, NOT_FOUND, NOT_OBJECT

COL_STRING, COL_STRING_CVT = 4, 5
MAX_COLS, MAX_PATH, MAX_KEYS, MAX_BYTES = 16, 16, 32, 1024
ROOT = 255
# why a table is refused (TablePlanError)
ERR_COLS, ERR_KIND, ERR_EMPTY_PATH, ERR_PATH_KEYS, ERR_KEYS, ERR_BYTES = range(1, 7)


class Refused(ValueError):
    def __init__(self, code):
        ValueError.__init__(self, code)
        self.code = code


class Node:
    def __init__(self, key, parent):
        self.key, self.parent, self.children, self.cols = key, parent, [], []


def plan(columns):
    """columns: [(path, kind)] -> (nodes, root_n); node: (key, parent or ROOT, first child, children, [columns that end here])"""
    if not 1 <= len(columns) <= MAX_COLS:
        raise Refused(ERR_COLS)
    n_keys = n_bytes = 0
    for path, kind in columns:  # (the first thing wrong in column order, like the C++)
        if not 0 <= kind <= COL_STRING_CVT:
            raise Refused(ERR_KIND)
        if len(path) == 0:
            raise Refused(ERR_EMPTY_PATH)
        if len(path) > MAX_PATH:
            raise Refused(ERR_PATH_KEYS)
        if n_keys + len(path) > MAX_KEYS:
            raise Refused(ERR_KEYS)
        n_keys += len(path)
        n_bytes += sum(len(k) for k in path)
        if n_bytes > MAX_BYTES:
            raise Refused(ERR_BYTES)
    root = Node(None, None)
    for c, (path, _) in enumerate(columns):
        cur = root
        for key in path:
            nxt = next((ch for ch in cur.children if ch.key == bytes(key)), None)
            if nxt is None:
                nxt = Node(bytes(key), cur)
                cur.children.append(nxt)
            cur = nxt
        cur.cols.append(c)
    order = list(root.children)
    first = {}
    q = 0
    while q < len(order):
        first[id(order[q])] = len(order)
        order.extend(order[q].children)
        q += 1
    num = {id(nd): j for j, nd in enumerate(order)}
    nodes = [(nd.key, ROOT if nd.parent is root else num[id(nd.parent)], first[id(nd)], len(nd.children), nd.cols) for nd in order]
    return nodes, len(root.children)


def walk(w, root, nodes, root_n, n_cols):
    """one record -> per column the tape index of the element's value, NOT_FOUND or NOT_OBJECT"""
    out = [None] * n_cols
    matched, notobj = set(), set()

    def below(j):
        _, _, b, n, _ = nodes[j]
        for ch in range(b, b + n):
            yield ch
            yield from below(ch)

    def scan(v, children):  # the object whose '{' is at v; -> nothing: the caller goes on behind it
        end = (w.t[v] & MASK) - 1
        i = v + 1
        while i < end and any(ch not in matched for ch in children):
            val = i + 2
            hit = next((ch for ch in children if ch not in matched and w.t[i + 1] == len(nodes[ch][0])
                        and w.string_at(i) == nodes[ch][0]), None)
            if hit is not None:
                matched.add(hit)
                _, _, b, n, cols = nodes[hit]
                for c in cols:
                    out[c] = val
                if n:
                    if chr(w.t[val] >> 56) == "{":
                        scan(val, range(b, b + n))
                    else:
                        notobj.update(below(hit))
            i = w.skip(val)

    if chr(w.t[root + 1] >> 56) != "{":
        notobj.update(range(len(nodes)))
    else:
        scan(root + 1, range(root_n))
    for j, (_, _, _, _, cols) in enumerate(nodes):
        if j not in matched:
            for c in cols:
                out[c] = NOT_OBJECT if j in notobj else NOT_FOUND
    assert None not in out
    return out


def indexes(w, columns):
    """-> [records][columns] of tape indexes / NOT_FOUND / NOT_OBJECT"""
    nodes, root_n = plan(columns)
    return [walk(w, root, nodes, root_n, len(columns)) for root in w.records()]


def table(w, columns):
    """-> per column what column_walk.column (values, statuses) / column_walk.string_column (offsets, data, statuses) return"""
    rows = indexes(w, columns)
    out = []
    for c, (_, kind) in enumerate(columns):
        if kind <= CW.COL_BOOL:
            vals, sts = [], []
            for row in rows:
                st, x = _path_status(row[c]), 0
                if st == CW.COL_OK:
                    st, x = CW.convert(w, row[c], kind)
                vals.append(x)
                sts.append(st)
            out.append((vals, sts))
        else:
            offs, parts, sts, at = [0], [], [], 0
            for row in rows:
                st, b = _path_status(row[c]), b""
                if st == CW.COL_OK:
                    st, b = CW.text(w, row[c], kind == COL_STRING_CVT)
                parts.append(b)
                at += len(b)
                offs.append(at)
                sts.append(st)
            out.append((offs, b"".join(parts), sts))
    return out


def _path_status(v):
    return CW.COL_NOT_OBJECT if v == NOT_OBJECT else CW.COL_NOT_FOUND if v == NOT_FOUND else CW.COL_OK


def single(w, path, kind):
    """the column on its own: column_walk's answer for (path, kind)"""
    if kind <= CW.COL_BOOL:
        return CW.column(w, path, kind)
    return CW.string_column(w, path, kind == COL_STRING_CVT)
