"""The selected rows as NDJSON text, restated serially on query_walk.Walk -- the checker of the device's sjhip_marshal_rows (test
infrastructure, like filter_rows_walk.py).

  row_text(w, v)              -> the compact JSON text of the row whose value is at tape index v
  marshal_rows(w, row_index)  -> (text, offsets): the rows' texts joined by '\n' (none behind the last), and the Arrow-style offsets
                                 sjhip_fetch_marshaled_rows hands out: offsets[i] = first byte of row i, offsets[n] = len(text) + 1
                                 (no rows: [0])

The formatter is the oracle's own (oracle_lib.marshal_json, Iter.MarshalJSON parsed_json.go:401-556): a row's words [v, end) -- end
= payload(tape[v]) for a container, v + 1 or 2 for a scalar -- are wrapped as root, '[', words, ']', root, with the payloads of the
row's brackets rebased as filter_rows_walk.py does and the strings left where they are (Strings.B and the message are handed over
unchanged); the text between the outer '[' and ']' is the row's.  So a scalar row is formatted by the oracle as well.

What this must equal is decided outside it (tests/test_marshal_rows_walk.py asks the oracle's marshal_json of whole documents)."""
import functools

import numpy as np

import oracle_lib as O
from filter_rows_walk import ROOT, _entries
from query_walk import MASK


def row_end(w, v):
    tag = chr(w.t[v] >> 56)
    if tag in "{[":
        return w.t[v] & MASK  # behind the matching close
    return v + 2 if tag in '"lud' else v + 1


def row_text(w, v):
    return _row_text(w, int(v))


@functools.lru_cache(maxsize=1 << 16)
def _row_text(w, v):
    """(a walk is hashed by identity and never edited: the text of the value at v is computed once per walk)"""
    end = row_end(w, v)
    n = end - v
    dw = 2 - v  # the row's first word becomes word 2
    tape = [ROOT | (n + 4), (ord("[") << 56) | (n + 3)]
    for i in _entries(w, v, end):
        word = w.t[i]
        tag = chr(word >> 56)
        if tag in "{}[]":
            word = (word & ~MASK) | ((word & MASK) + dw)
        tape.append(word)
        if tag in '"lud':
            tape.append(w.t[i + 1])
    tape += [(ord("]") << 56) | 1, ROOT | 0]
    assert len(tape) == n + 4
    rc, text = O.marshal_json(np.array(tape, dtype=np.uint64), np.frombuffer(w.s, dtype=np.uint8), w.m)
    assert rc == 0 and text[:1] == b"[" and text[-1:] == b"]", (rc, text[:40])
    return text[1:-1]


def marshal_rows(w, row_index):
    texts = [row_text(w, v) for v in row_index]
    offsets, at = [], 0
    for t in texts:
        offsets.append(at)
        at += len(t) + 1
    offsets.append(at if texts else 0)
    return b"\n".join(texts), offsets
