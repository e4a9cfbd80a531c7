"""GPU: the products that are built part by part and joined by their fetch -- the string column, the list columns and the table --
on a sharded result in which whole shards contribute NOTHING: no bytes and no elements.  The random documents of the other
sharded tests give every shard something, so offsets rebased over the wrong prefix (records for elements, elements for bytes)
can pass there; here a shard without values lies in front of shards with values (stretches A, B, C: the path is absent in B),
and in the second document the first and the last shards are the empty ones (B, A, B).  Everything is compared bit for bit with
the same calls on the same document parsed whole.

The document is the smallest the environment hook allows: nd_too_big (parse_api.hip) looks at SJHIP_ND_LIMIT_BYTES for messages
of more than 1 MiB only, so ~1.2 MiB, a limit of 1 MiB and shards of 256 KiB: five shards, cut right behind the first newline
at or after k * len / 5 (multi_api.hip multi_parse).  shard_spans restates that rule, and the tests check on the document itself
that the construction holds."""
import numpy as np
import pytest

import column_walk as CW
import fixtures
import list_walk as LW
import table_walk as TW

gpu = pytest.mark.gpu  # (test_the_construction_holds needs none)

LIMIT, SHARD = 1 << 20, 256 << 10
KIB = 1 << 10


def stretch(first, nbytes, values):
    """records of ~100 bytes from number `first` on, nbytes in all; with `values` the paths s, t, n and x hold something"""
    lines, size, r = [], 0, first
    while size < nbytes:
        if values:
            line = '{"id":%d,"s":"v%d%s","t":["a%d","%s"],"n":[%d,2.5,%d],"x":%d,"pad":"%s"}' % (
                1000000 + r, r, "y" * (r % 5), r % 10, "z" * (r % 4), r, r % 7, r * 3 - 5, "p" * 20)
        else:
            line = '{"id":%d,"pad":"%s"}' % (1000000 + r, "p" * (70 + r % 9))
        lines.append(line)
        size += len(line) + 1
        r += 1
    return lines


def document(order):
    lines = []
    for values, nbytes in order:
        lines += stretch(len(lines), nbytes, values)
    return "\n".join(lines).encode()


def shard_spans(doc):
    n = (len(doc) + SHARD - 1) // SHARD
    cuts = [0]
    for k in range(1, n):
        cuts.append(doc.index(b"\n", max(len(doc) * k // n, cuts[-1])) + 1)
    cuts.append(len(doc))
    return [doc[a:b] for a, b in zip(cuts, cuts[1:])]


ABC = document([(True, 300 * KIB), (False, 600 * KIB), (True, 300 * KIB)])
BAB = document([(False, 400 * KIB), (True, 400 * KIB), (False, 400 * KIB)])
DOCS = {"ABC": ABC, "BAB": BAB}


def test_the_construction_holds():
    import oracle_lib as O
    for name, doc in DOCS.items():
        assert O.parse(doc, ndjson=True).rc == 0, name
        assert LIMIT < len(doc) < LIMIT + 300 * KIB, name
        has = [b'"s":' in s for s in shard_spans(doc)]
        assert len(has) == 5, name
        if name == "ABC":  # a shard wholly inside B, with values in front of it and behind it
            assert has[0] and not has[2] and has[4], has
        else:  # the first and the last shards are the empty ones
            assert not has[0] and has[2] and not has[4], has


_ctxs = {}


def contexts(name):
    """(the document parsed whole, the document parsed in shards), shared by the tests and left as they are"""
    import sjhip
    if name not in _ctxs:
        one, many = sjhip.Context(0), sjhip.Context(0)
        one.parse(DOCS[name], ndjson=True)
        with fixtures.nd_shard_limits(LIMIT, SHARD):
            many.parse(DOCS[name], ndjson=True)
        _ctxs[name] = (one, many)
    return _ctxs[name]


def same(got, want, what):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        if isinstance(w, np.ndarray):
            assert g.dtype == w.dtype and g.shape == w.shape, (what, k)
            bits = np.uint8 if w.dtype.itemsize == 1 else np.uint64
            assert np.array_equal(g.view(bits), w.view(bits)), (what, k)
        else:
            assert g == w, (what, k)


def offsets_end_at(off, total, what):
    assert off.dtype == np.uint64 and len(off) >= 1 and int(off[0]) == 0, what
    assert np.all(off[1:] >= off[:-1]), what
    assert int(off[-1]) == total, what


@gpu
@pytest.mark.parametrize("name", list(DOCS))
def test_string_column(name):
    one, many = contexts(name)
    for cvt in (False, True):
        want, got = one.extract_path_strings((b"s",), cvt=cvt), many.extract_path_strings((b"s",), cvt=cvt)
        same(got, want, (name, cvt))
        off, data, st = got
        offsets_end_at(off, len(data), (name, cvt))
        assert len(data) > 0 and set(st.tolist()) == {CW.COL_OK, CW.COL_NOT_FOUND}


@gpu
@pytest.mark.parametrize("name", list(DOCS))
def test_list_columns(name):
    one, many = contexts(name)
    want, got = one.extract_path_list((b"n",), LW.COL_FLOAT), many.extract_path_list((b"n",), LW.COL_FLOAT)
    same(got, want, (name, "numbers"))
    off, vals, st = got
    offsets_end_at(off, len(vals), (name, "numbers"))
    assert len(vals) > 0 and len(off) == len(st) + 1
    for cvt in (False, True):
        want, got = one.extract_path_list_strings((b"t",), cvt=cvt), many.extract_path_list_strings((b"t",), cvt=cvt)
        same(got, want, (name, "strings", cvt))
        off, soff, data, st = got
        offsets_end_at(off, len(soff) - 1, (name, "list offsets", cvt))
        offsets_end_at(soff, len(data), (name, "string offsets", cvt))
        assert len(data) > 0 and len(off) == len(st) + 1


@gpu
@pytest.mark.parametrize("name", list(DOCS))
def test_table(name):
    one, many = contexts(name)
    columns = [((b"x",), CW.COL_INT), ((b"s",), TW.COL_STRING)]
    want, got = one.extract_table(columns), many.extract_table(columns)
    assert len(got) == 2
    same(got[0], want[0], (name, "x"))
    same(got[1], want[1], (name, "s"))
    off, data, st = got[1]
    offsets_end_at(off, len(data), (name, "s"))
    assert len(data) > 0 and len(got[0][0]) == len(st) == len(off) - 1
    # ... and the table's string column is the single string column
    same(got[1], many.extract_path_strings((b"s",)), (name, "single"))
