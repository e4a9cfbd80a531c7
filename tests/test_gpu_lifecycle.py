"""GPU: the lifecycle of a context's result and of the products derived from it (csrc/sj_result.h; DESIGN.md 3a, the table
"call x product"): after a product has been made and fetched, an interloping call either leaves it alone -- the same fetch returns
the same bytes -- or drops it -- the fetch is SJHIP_ERR_ARG; on a whole result, on a sharded one, and after every parse call that
returns early."""
import ctypes as C
import os
import random

import numpy as np
import pytest

from test_gpu_parse import ctx  # noqa: F401

pytestmark = pytest.mark.gpu

ERR_ARG = 5
PRODUCTS = ["filtered", "serialized", "marshaled", "column", "list_numbers", "list_strings"]


def make_doc(records, seed=41):
    rnd = random.Random(seed)
    return "\n".join('{"Make":"%s","tags":[%s],"xs":[%s]}' % (
        rnd.choice(["HOND", "TOYT", "x" * 50]), ",".join('"t%d"' % rnd.randrange(99) for _ in range(rnd.randint(0, 5))),
        ",".join(str(rnd.randrange(1000)) for _ in range(rnd.randint(0, 9)))) for _ in range(records)).encode()


DOC = make_doc(400)


def L():
    import sjhip
    return sjhip._lib.lib()


def make(c, product):
    """Builds the product on the device; -> what its fetch needs to know (sizes)."""
    if product == "filtered":
        n, tl, sl = C.c_uint64(0), C.c_size_t(0), C.c_size_t(0)
        c._check(L().sjhip_filter_where(c._h, b"Make", 4, b"HOND", 4, C.byref(n), C.byref(tl), C.byref(sl)))
        assert n.value > 0
        return tl.value, sl.value
    if product == "serialized":
        return (c.serialize(fetch=False)["stream"],)
    if product == "marshaled":
        return (c.marshal_json(fetch=False),)
    if product == "column":
        return c.extract_path_strings((b"Make",), fetch=False)
    if product == "list_numbers":
        return c.extract_path_list((b"xs",), c.COL_FLOAT, fetch=False)
    assert product == "list_strings"
    return c.extract_path_list_strings((b"tags",), fetch=False)


def fetch(c, product, sizes=None, room=1 << 20):
    """The raw fetch of the product into buffers of `room` bytes each (more than any product of these documents, whatever the
    library believes to hold) -> (return code, the fetched bytes)."""
    bufs = [np.zeros(room, dtype=np.uint8) for _ in range(4)]
    p = [b.ctypes.data for b in bufs]
    if product == "filtered":
        rc = L().sjhip_fetch_filtered(c._h, p[0], p[1])
        cut = sizes and (sizes[0] * 8, sizes[1])
    elif product == "serialized":
        got = C.c_size_t(0)
        rc = L().sjhip_fetch_serialized(c._h, p[0], room, C.byref(got))
        assert rc != 0 or got.value == sizes[0]
        cut = sizes
    elif product == "marshaled":
        rc = L().sjhip_fetch_marshaled(c._h, p[0])
        cut = sizes
    elif product == "column":
        rc = L().sjhip_fetch_path_strings(c._h, p[0], p[1], p[2])
        cut = sizes and (8 * (sizes[0] + 1), sizes[1], sizes[0])
    elif product == "list_numbers":
        rc = L().sjhip_fetch_path_list(c._h, p[0], p[1], p[2])
        cut = sizes and (8 * (sizes[0] + 1), 8 * sizes[1], sizes[0])
    else:
        rc = L().sjhip_fetch_path_list_strings(c._h, p[0], p[1], p[2], p[3])
        cut = sizes and (8 * (sizes[0] + 1), 8 * (sizes[1] + 1), sizes[2], sizes[0])
    if rc != 0:
        return rc, None
    assert all(n <= room for n in cut)
    return 0, tuple(b[:n].tobytes() for b, n in zip(bufs, cut))


def count(c):
    n = C.c_uint64(0)
    return L().sjhip_count_where(c._h, b"Make", 4, b"HOND", 4, C.byref(n)), n.value


_STREAM = []


def serialized_stream():
    if not _STREAM:
        import sjhip
        other = sjhip.Context(0)
        other.parse(b'{"a":["b",1]}')
        _STREAM.append(other.serialize().copy())
        other.close()
    return _STREAM[0]


INTERLOPERS = {
    "filtered": lambda c: make(c, "filtered"), "serialized": lambda c: make(c, "serialized"), "marshaled": lambda c: make(c, "marshaled"),
    "column": lambda c: make(c, "column"), "list_numbers": lambda c: make(c, "list_numbers"), "list_strings": lambda c: make(c, "list_strings"),
    "count_query": lambda c: c.count_where(b"Make", b"TOYT"), "path_query": lambda c: c.find_path(b"xs"),
    "parse": lambda c: c.parse(b'{"Make":"HOND"}\n{"Make":"x"}', ndjson=True), "stage1_only": lambda c: c.stage1(b'{"a":[1,2]}'),
    "trim": lambda c: c.trim(), "deserialize": lambda c: c.deserialize(serialized_stream()),
}
# the products a call leaves alone; every other cell of its row is "dropped"
TENANTS = {"filtered", "serialized", "marshaled"}
COLUMNS = {"column", "list_numbers", "list_strings"}
SURVIVES = {
    "filtered": COLUMNS, "serialized": COLUMNS, "marshaled": COLUMNS, "column": TENANTS | COLUMNS,
    "list_numbers": TENANTS | {"column"}, "list_strings": TENANTS | {"column"}, "count_query": TENANTS | COLUMNS,
    "path_query": TENANTS | COLUMNS, "parse": set(), "stage1_only": set(), "trim": set(), "deserialize": set(),
}
MATRIX = [(p, i) for p in PRODUCTS for i in INTERLOPERS if i != p]


def check_cell(c, product, interloper):
    sizes = make(c, product)
    rc, first = fetch(c, product, sizes)
    assert rc == 0 and any(len(b) for b in first)
    INTERLOPERS[interloper](c)
    rc, again = fetch(c, product, sizes)
    if product in SURVIVES[interloper]:
        assert rc == 0 and again == first, (product, interloper)
    else:
        assert rc == ERR_ARG, (product, interloper, rc)


@pytest.mark.parametrize("product,interloper", MATRIX, ids=["%s-%s" % m for m in MATRIX])
def test_matrix(ctx, product, interloper):
    ctx.parse(DOC, ndjson=True, key_flags=True)
    check_cell(ctx, product, interloper)


# ---- parse calls that return early: the uniform rule --------------------------------------------------------------------------
def batch(c, docs, flags):
    arrs = [np.frombuffer(d, dtype=np.uint8) for d in docs]
    n = len(arrs)
    ptrs = (C.c_void_p * max(n, 1))(*[a.ctypes.data if a.size else None for a in arrs])
    lens = (C.c_size_t * max(n, 1))(*[a.size for a in arrs])
    tl, sl = C.c_size_t(0), C.c_size_t(0)
    return L().sjhip_parse_batch(c._h, ptrs, lens, n, flags, C.byref(tl), C.byref(sl))


def raw_parse(c, data):
    a = np.frombuffer(data, dtype=np.uint8)
    z = [C.c_size_t(0) for _ in range(4)]
    return L().sjhip_parse(c._h, a.ctypes.data if a.size else None, a.size, 2, *[C.byref(x) for x in z])


FAILING_PARSES = {  # -> the call's return code
    "parse_empty": (lambda c: raw_parse(c, b""), 1), "parse_whitespace": (lambda c: raw_parse(c, b" \n\t \r\n"), 1),
    "batch_without_copy_strings": (lambda c: batch(c, [b'{"a":1}'], 0), ERR_ARG), "batch_of_no_documents": (lambda c: batch(c, [], 2), 1),
    "batch_with_a_scalar_document": (lambda c: batch(c, [b'{"a":1}', b"17", b"[2]"], 2), 1),
    "batch_with_an_empty_document": (lambda c: batch(c, [b'{"a":1}', b"  ", b"[2]"], 2), 1),
    "shard_begin_without_out_pointers": (lambda c: L().sjhip_parse_shard_begin(c._h, None, 1, 3, None, None), ERR_ARG),
}


@pytest.mark.parametrize("product", PRODUCTS)
@pytest.mark.parametrize("call", list(FAILING_PARSES))
def test_a_failed_parse_drops_everything(ctx, call, product):
    """Before the lifecycle state these early returns cleared the tape length and little else: the products of the parse before
    them could still be fetched."""
    ctx.parse(DOC, ndjson=True, key_flags=True)
    sizes = make(ctx, product)
    assert fetch(ctx, product, sizes)[0] == 0 and count(ctx)[0] == 0
    fail, code = FAILING_PARSES[call]
    assert fail(ctx) == code
    for p in PRODUCTS:
        assert fetch(ctx, p)[0] == ERR_ARG, (call, product, p)
    assert count(ctx)[0] == ERR_ARG and "no parse result on the device" in ctx.last_error()
    ctx.parse(DOC, ndjson=True)  # ... and the context goes on as usual
    assert count(ctx) == (0, DOC.count(b'"HOND"'))


# ---- a sharded result ---------------------------------------------------------------------------------------------------------
SHARDED_PRODUCTS = ["marshaled", "column", "list_numbers", "list_strings"]
SHARDED_MATRIX = [(p, i) for p in SHARDED_PRODUCTS for i in INTERLOPERS if i != p and i not in ("filtered", "serialized")]


@pytest.fixture(scope="module")
def sharded():
    """A context and a document of a little over 2 MiB that it parses in shards of 1 MiB."""
    import sjhip
    doc = make_doc(30000, seed=42)
    assert (2 << 20) < len(doc) < (3 << 20)
    c = sjhip.Context(0)

    def parse():
        os.environ["SJHIP_ND_LIMIT_BYTES"] = str(2 << 20)
        os.environ["SJHIP_ND_SHARD_BYTES"] = str(1 << 20)
        try:
            c.parse(doc, ndjson=True, key_flags=True)
        finally:
            del os.environ["SJHIP_ND_LIMIT_BYTES"], os.environ["SJHIP_ND_SHARD_BYTES"]
    yield c, parse, doc
    c.close()


@pytest.mark.parametrize("product,interloper", SHARDED_MATRIX, ids=["%s-%s" % m for m in SHARDED_MATRIX])
def test_matrix_on_a_sharded_result(sharded, product, interloper):
    c, parse, doc = sharded
    parse()
    sizes = make(c, product)
    rc, first = fetch(c, product, sizes, room=8 << 20)
    assert rc == 0 and any(len(b) for b in first)
    INTERLOPERS[interloper](c)
    rc, again = fetch(c, product, sizes, room=8 << 20)
    if product in SURVIVES[interloper]:
        assert rc == 0 and again == first, (product, interloper)
    else:
        assert rc == ERR_ARG, (product, interloper, rc)


def test_the_sharded_result_is_sharded(sharded):
    """... and the filter and the serializer, which work on the result of one context, refuse it: the filter touches nothing, the
    serializer gives up the tenants it may replace (its own and the MarshalJSON text) before its checks, the columns stay."""
    import sjhip
    c, parse, doc = sharded
    parse()
    assert c.count_where(b"Make", b"HOND") == doc.count(b'"HOND"')
    sizes = make(c, "marshaled")
    rc, first = fetch(c, "marshaled", sizes, room=8 << 20)
    assert rc == 0
    with pytest.raises(sjhip.ParseError) as e:
        c.filter_where(b"Make", b"HOND")
    assert e.value.code == ERR_ARG and "parsed shard by shard" in str(e.value)
    assert fetch(c, "marshaled", sizes, room=8 << 20) == (0, first)
    col = make(c, "column")
    rc, first_col = fetch(c, "column", col, room=8 << 20)
    assert rc == 0
    with pytest.raises(sjhip.ParseError) as e:
        c.serialize()
    assert e.value.code == ERR_ARG and "parsed shard by shard" in str(e.value)
    assert fetch(c, "marshaled", sizes, room=8 << 20)[0] == ERR_ARG
    assert fetch(c, "column", col, room=8 << 20) == (0, first_col)


def test_a_refused_product_call_gives_up_its_own_product_only(ctx):
    """A result parsed without copied strings: the filter and the serializer refuse it, MarshalJSON works.  A refused filter
    touches nothing; a refused serialize gives up the serialized stream and the MarshalJSON text, nothing else."""
    import sjhip
    ctx.parse(DOC, ndjson=True, copy_strings=False)
    text = make(ctx, "marshaled")
    col = make(ctx, "column")
    first = fetch(ctx, "marshaled", text)
    first_col = fetch(ctx, "column", col)
    assert first[0] == 0 and first_col[0] == 0
    with pytest.raises(sjhip.ParseError) as e:
        ctx.filter_where(b"Make", b"HOND")
    assert e.value.code == ERR_ARG and "SJHIP_FLAG_COPY_STRINGS" in str(e.value)
    assert fetch(ctx, "marshaled", text) == first
    with pytest.raises(sjhip.ParseError) as e:
        ctx.serialize()
    assert e.value.code == ERR_ARG and "SJHIP_FLAG_COPY_STRINGS" in str(e.value)
    assert fetch(ctx, "marshaled", text)[0] == ERR_ARG
    assert fetch(ctx, "column", col) == first_col
    # ... and on a result with copied strings, a filter whose key is refused leaves the serialized stream alone
    ctx.parse(DOC, ndjson=True)
    stream = make(ctx, "serialized")
    first = fetch(ctx, "serialized", stream)
    with pytest.raises(sjhip.ParseError):
        ctx.filter_where(b"k" * 5000, b"HOND")
    assert first[0] == 0 and fetch(ctx, "serialized", stream) == first
