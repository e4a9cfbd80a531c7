"""The selected rows projected onto k paths as NDJSON text, restated serially on query_walk.Walk -- the checker of the device's
sjhip_marshal_rows_paths (test infrastructure, like marshal_rows_walk.py).

  indexes(w, v, columns)                     -> per column the tape index of the element / NOT_FOUND / NOT_OBJECT in the row at v:
                                                table_walk's plan and walk over the columns that have keys, the row itself for the others
  name_text(name)                            -> '"' + escapeBytes(name) + '"': the oracle's marshal of a one-string tape built by hand
  row_text(w, v, columns, names, nulls)      -> '{' + the present columns, joined by ',' + '}'
  project_rows(w, row_index, columns, names=None, nulls=False)
                                             -> (text, offsets) shaped like marshal_rows_walk.marshal_rows

The cell text is marshal_rows_walk.row_text's (the oracle's formatter).  What this must equal is decided outside it
(tests/test_project_rows_walk.py)."""
import functools

import numpy as np

import marshal_rows_walk as MW
import oracle_lib as O
import table_walk as TW
from filter_rows_walk import ROOT
from query_walk import NOT_FOUND, NOT_OBJECT, STRINGBUFBIT

MAX_NAME_BYTES = 1024


def indexes(w, v, columns):
    v = int(v)
    out = [v] * len(columns)
    keyed = [c for c, path in enumerate(columns) if len(path)]
    if keyed:
        nodes, root_n = TW.plan([(columns[c], 0) for c in keyed])
        for c, x in zip(keyed, TW.walk(w, v - 1, nodes, root_n, len(keyed))):  # (walk looks at the value behind `root`)
            out[c] = x
    return out


@functools.lru_cache(maxsize=None)
def name_text(name):
    tape = [ROOT | 6, (ord("[") << 56) | 5, (ord('"') << 56) | STRINGBUFBIT, len(name), (ord("]") << 56) | 1, ROOT | 0]
    rc, text = O.marshal_json(np.array(tape, dtype=np.uint64), np.frombuffer(name, dtype=np.uint8), b"")
    assert rc == 0 and text[:2] == b'["' and text[-2:] == b'"]', (rc, text[:40])
    return text[1:-1]


def column_names(columns, names):
    if names is None:
        assert all(len(path) for path in columns)
        return [bytes(path[-1]) for path in columns]
    assert len(names) == len(columns)
    return [bytes(x) for x in names]


def row_text(w, v, columns, names=None, nulls=False):
    parts = []
    for x, name in zip(indexes(w, v, columns), column_names(columns, names)):
        if x in (NOT_FOUND, NOT_OBJECT):
            if nulls:
                parts.append(name_text(name) + b":null")
            continue
        parts.append(name_text(name) + b":" + MW.row_text(w, x))
    return b"{" + b",".join(parts) + b"}"


def project_rows(w, row_index, columns, names=None, nulls=False):
    texts = [row_text(w, v, columns, names, nulls) for v in row_index]
    offsets, at = [], 0
    for t in texts:
        offsets.append(at)
        at += len(t) + 1
    offsets.append(at if texts else 0)
    return b"\n".join(texts), offsets
