"""The selected rows as a self-contained (Tape, Strings.B), restated serially on query_walk.Walk -- the checker of the device's
sjhip_filter_rows (test infrastructure, like rows_walk.py).

  filter_rows(w, row_index) -> (tape, strings, skipped)

Every row whose value is an object or an array becomes a record: an opening root word 'r' << 56 | index behind its closing root,
the row's words [v, payload(tape[v])) -- the payload of every { } [ ] word moved by (new index - old index), the payload of every
string word moved to the new Strings.B, the second words of strings and numbers as they are --, a closing root word
'r' << 56 | index of the opening root.  The walk goes entry by entry (a tag word, then its raw word if it has one), so a raw
word is never looked at as a tag.  The new Strings.B is the rows' bytes end to end; a row owns the bytes from the offset of its
first string to the end of its last one.  A scalar row has no record: it is left out and counted.

What this must equal is decided outside it: ParseND with copied strings of the document whose lines are the texts of the rows
(tests/test_filter_rows_walk.py asks the oracle)."""
from query_walk import MASK, STRINGBUFBIT

ROOT = ord("r") << 56


def filter_rows(w, row_index):
    tape, strings, skipped = [], bytearray(), 0
    for v in row_index:
        v = int(v)
        if chr(w.t[v] >> 56) not in "{[":
            skipped += 1
            continue
        end = w.t[v] & MASK  # behind the matching close
        na = len(tape)
        dw = na + 1 - v
        first, last_end = None, 0
        for i in _entries(w, v, end):  # the row's Strings.B range
            if chr(w.t[i] >> 56) == '"':
                off = w.t[i] & (STRINGBUFBIT - 1)
                assert w.t[i] & STRINGBUFBIT, "filter_rows needs copied strings"
                if first is None:
                    first = off
                last_end = off + w.t[i + 1]
        ds = len(strings) - first if first is not None else 0
        tape.append(ROOT | (na + (end - v) + 2))
        for i in _entries(w, v, end):
            word = w.t[i]
            tag = chr(word >> 56)
            if tag in "{}[]":
                word = (word & ~MASK) | ((word & MASK) + dw)
            elif tag == '"':
                word += ds
            tape.append(word)
            if tag in '"lud':
                tape.append(w.t[i + 1])
        tape.append(ROOT | na)
        if first is not None:
            strings += w.s[first:last_end]
    return tape, bytes(strings), skipped


def _entries(w, v, end):
    i = v
    while i < end:
        yield i
        i += 2 if chr(w.t[i] >> 56) in '"lud' else 1
