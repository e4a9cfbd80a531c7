"""GPU: the string pass (csrc/sj_strings.h, the string half of csrc/stage2.hip) with a hazard exactly on every cut of its
work -- chunk, unit, block, first and last seam, message end, and the 64-unit steps of the selective copy's walks.  The
documents are those of tests/str_geometry.py; tests/test_str_geometry.py checks on the CPU that they cover what they
claim and that the model used here agrees with the oracle.

Every document goes through check() of test_gpu_parse: both copy modes, Tape and Strings.B bit-identical to the oracle's,
the error class equal.  For plain documents Strings.B must also be what the independent model expects."""
import numpy as np
import pytest

import golden_util as GU
import oracle_lib as O
import str_geometry as S
from test_gpu_parse import check, ctx  # noqa: F401

pytestmark = pytest.mark.gpu


def _whole(ctx, d):
    check(ctx, d.data, d.nd, d.name)
    if d.plain:
        for copy in (True, False):
            pj = ctx.parse(d.data, ndjson=d.nd, copy_strings=copy)
            assert bytes(pj.Strings) == S.expected_strings(d.data, copy), (d.name, copy)


def _marshal(ctx, d):
    """the marshal reads Strings.B by the offsets under test (key flags on, as MarshalJSON needs them)"""
    ref = O.parse(d.data, ndjson=d.nd, copy_strings=True)
    assert ref.rc == 0, d.name
    msg = d.data[ref.msg_off:ref.msg_off + ref.msg_len]
    pj = ctx.parse(d.data, ndjson=d.nd, copy_strings=True, key_flags=True)
    assert bytes(pj.Strings) == S.expected_strings(d.data, True), d.name
    rc, want = O.marshal_json(ref.tape, ref.strings, msg)
    assert rc == 0 and ctx.marshal_json() == want, d.name


@pytest.mark.parametrize("nd", [False, True])
def test_rotation_documents(ctx, nd):
    for d in S.rotation_docs(nd):
        _whole(ctx, d)
        _marshal(ctx, d)


@pytest.mark.parametrize("lead", [1, 63])
def test_chunk_seams_from_an_unaligned_device_pointer(ctx, lead):
    """parse_device from a device buffer: chunks count from the 64-byte aligned base in front of the pointer"""
    import torch
    for nd in (False, True):
        d = S.lead_doc(lead, nd)
        doc = d.data
        dev = torch.zeros(len(doc) + 512, dtype=torch.uint8, device="cuda:0")
        dev[lead:lead + len(doc)].copy_(torch.frombuffer(bytearray(doc), dtype=torch.uint8))
        torch.cuda.synchronize()
        for copy in (True, False):
            ref = O.parse(doc, ndjson=nd, copy_strings=copy)
            assert ref.rc == 0 and ref.msg_off == 0 and ref.msg_len == len(doc)
            tl, sl = ctx.parse_device(dev.data_ptr() + lead, len(doc), ndjson=nd, copy_strings=copy)
            tape, strings = ctx.fetch(tl, sl)
            assert np.array_equal(tape, ref.tape), (d.name, copy)
            assert np.array_equal(strings, ref.strings), (d.name, copy)
            assert bytes(strings) == S.expected_strings(doc, copy), (d.name, copy)
        _whole(ctx, d)  # the same bytes from the host (lead 0): other seams, nothing lost


def test_error_documents(ctx):
    for d in S.error_docs():
        assert O.parse(d.data).rc != 0, d.name
        check(ctx, d.data, False, d.name)


def test_golden_bodies_on_the_seams(ctx):
    bodies = [bytes.fromhex(r["str_hex"]) for r in GU.load("strings")]
    for d in S.quirk_docs(bodies):
        check(ctx, d.data, False, d.name)


def test_compaction_documents(ctx):
    for d in list(S.compaction_docs()) + [S.unit_count_doc()]:
        _whole(ctx, d)


def test_patch_documents(ctx):
    for d in S.patch_docs():
        _whole(ctx, d)


def test_selective_four_strings_in_a_chunk(ctx):
    for d in S.sel_chunk_docs():
        _whole(ctx, d)


def _one(ctx, d, copy, refs):
    key = (d.name, copy)
    if key not in refs:
        refs[key] = O.parse(d.data, ndjson=d.nd, copy_strings=copy)
        assert refs[key].rc == 0 and refs[key].strings.tobytes() == S.expected_strings(d.data, copy), key
    pj = ctx.parse(d.data, ndjson=d.nd, copy_strings=copy)
    assert np.array_equal(pj.Tape, refs[key].tape), key
    assert np.array_equal(pj.Strings, refs[key].strings), key


def test_selective_long_strings_alternating_on_one_context(ctx):
    """large, small, large on one context: a stale unit_copy / unit_tq / soff of the parse before would show; copy mode
    right after no-copy mode of the same document and the other way round"""
    docs = list(S.sel_long_docs())
    assert len(docs) == sum(S.sel_place_applies(n, p) for n in S.SEL_UNITS for p in S.SEL_PLACES) == 46
    small = list(S.sel_message_docs()) + list(S.sel_quote_docs())
    big_first = sorted(docs, key=lambda d: -len(d.data))
    refs = {}
    for i, d in enumerate(big_first):
        check(ctx, d.data, False, d.name)
        s = small[i % len(small)]
        t = big_first[(i + 7) % len(big_first)]
        for order in ((False, True), (True, False)):
            for x in (d, s, t):
                for copy in order:
                    _one(ctx, x, copy, refs)
            if i % 4:
                break  # (every fourth document in both orders, the others no-copy first)


def test_selective_messages_and_quotes_on_the_unit_edge(ctx):
    docs = list(S.sel_message_docs()) + list(S.sel_quote_docs())
    for d in docs:
        _whole(ctx, d)
    refs = {}
    for copy_first in (False, True):  # the no_escapes shortcut between parses that copy, and the other way round
        for a in docs:
            for b in docs[:4]:
                _one(ctx, a, copy_first, refs)
                _one(ctx, b, not copy_first, refs)
                _one(ctx, b, copy_first, refs)


def test_rotation_documents_beyond_the_small_path(ctx):
    d = S.big_doc()
    assert len(d.data) > 4 << 20
    _whole(ctx, d)
