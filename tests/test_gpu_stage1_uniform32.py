"""GPU tests of the 32-bit wave-uniform state of the stage-1 tile loop (run with -m gpu on an MI355X; stage1.hip tile_unit,
ticket_pack, msg_at): plain stage 1 keeps unit numbers and byte offsets in 32 bits -- its launches refuse lead + len >= 2^32 --
and a grouped launch resolves the message of a ticket once, where the ticket is drawn.  The cases sit where that can go wrong:
the top of the 32-bit range (the end of the top unit is 2^32), and groups whose consecutive tickets belong to three messages."""
import numpy as np
import pytest

import oracle_lib as O
import workloads
from test_gpu_stage1_group import G, TILE, UNIT, Msg, burst, doc

pytestmark = pytest.mark.gpu

TOP = 1 << 32
TAIL = 5 * UNIT   # bytes in front of the message's end that hold more than blanks
CAP = 4096        # words of the position buffer (a message of blanks has few structurals)
SENTINEL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def ctx():
    import sjhip
    assert sjhip.supported(), "gfx950 device required"
    c = sjhip.Context(0)
    yield c
    c.close()


# ---- the top of the 32-bit range -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def blanks():
    """2^32 + 64 blanks on the device (built there: no host copy), 64-byte aligned; every case puts them back"""
    import torch
    dev = torch.full((TOP + 64,), 0x20, dtype=torch.uint8, device="cuda:0")
    assert dev.data_ptr() % 64 == 0
    return dev


def tail_bytes(end):
    """the last TAIL bytes of a message that ends at buffer offset `end`: blanks, a handful of structurals and one string with
    an escaped quote in the last three units, more across the unit boundary at 2^32 - 4096 where the message reaches it, ']' last"""
    t = bytearray(b" " * TAIL)

    def put(at, s):  # at: offset from the END of the message
        assert 0 < at <= TAIL and at - len(s) >= 1
        t[TAIL - at:TAIL - at + len(s)] = s

    put(3 * UNIT - 100, b'{"k":"a\\"b",')
    put(2 * UNIT + 3, b'"cd":[1,2],')       # (crosses a unit boundary of a message that ends on one)
    put(UNIT + 70, b'"e\\\\":true,')
    put(200, b'"f":{"g":null}}')
    edge = end - (TOP - UNIT)                # the unit boundary at 2^32 - 4096, as an offset from the end
    if 64 < edge < TAIL - 64 and not (180 <= edge <= 230):
        clear = all(t[TAIL - edge - 8 + i] == 0x20 for i in range(24))
        if clear:
            put(edge + 5, b'"h\\"i":[3,4],')  # quote, escape and brackets on both sides of the boundary
    t[TAIL - 1:TAIL] = b"]"
    return bytes(t)


def expected(tail, length):
    """count, verdict and positions follow from the construction: '[' first, blanks, the tail -- blanks change no state, so the
    oracle's stage 1 of '[' + tail gives them, its positions behind the first moved to the end of the message"""
    ok, pos = O.stage1(b"[" + tail)
    assert pos[0] == 0 and len(pos) > 20
    want = pos.astype(np.uint64)
    want[1:] += np.uint64(length - len(tail) - 1)
    assert want[-1] == length - 1 and want[-1] < TOP
    return ok, want.astype(np.uint32)


TOP_LENGTHS = {"largest": 0xffffffbf, "one unit shorter": 0xffffffbf - UNIT, "ends on a unit boundary": None}


@pytest.mark.parametrize("lead", [0, 63])
@pytest.mark.parametrize("which", list(TOP_LENGTHS))
def test_top_of_the_32_bit_range(ctx, blanks, which, lead):
    import torch
    length = TOP_LENGTHS[which] if TOP_LENGTHS[which] is not None else (TOP - UNIT) - lead
    end = lead + length
    assert end < TOP and (which != "ends on a unit boundary" or end % UNIT == 0)
    tail = tail_bytes(end)
    ok_ref, want = expected(tail, length)
    pos = torch.empty(CAP + 64, dtype=torch.int32, device="cuda:0")
    small = [Msg(doc(100)), Msg(doc(UNIT + 1), lead=63)]
    for m in small:
        m.run_single(ctx)
    try:
        blanks[end - TAIL:end].copy_(torch.frombuffer(bytearray(tail), dtype=torch.uint8))
        blanks[lead] = ord("[")
        ptr = blanks.data_ptr() + lead

        def check(ok, n, where):
            got = pos.cpu().numpy().view(np.uint32)
            assert np.all(got[CAP:] == SENTINEL), where
            assert (ok, n) == (ok_ref, len(want)), (where, ok, n, ok_ref, len(want))
            assert np.array_equal(got[:n][-64:], want[-64:]) and np.array_equal(got[:n], want), where

        pos.fill_(SENTINEL)
        torch.cuda.synchronize()
        ok, n = ctx.stage1_device(ptr, length, pos.data_ptr(), CAP)
        check(ok, n, "stage1_device")
        # ... and as the last message of a queued group
        pos.fill_(SENTINEL)
        for m in small:
            m.reset()
        torch.cuda.synchronize()
        for slot, m in enumerate(small):
            ctx.stage1_queue(m.ptr(), len(m.data), m.pos.data_ptr(), m.cap, slot)
        ctx.stage1_queue(ptr, length, pos.data_ptr(), CAP, len(small))
        ctx.stage1_wait()
        for slot, m in enumerate(small):
            ok, n = ctx.stage1_result(slot, len(m.data))
            m.check(ok, n, ("in front of the large message", slot))
        ok, n = ctx.stage1_result(len(small), length)
        check(ok, n, "last message of a group")
    finally:
        blanks[end - TAIL:end] = 0x20
        blanks[lead] = 0x20
        torch.cuda.synchronize()


def test_a_message_of_4_gib_minus_64_is_still_refused(ctx, blanks):
    import torch
    pos = torch.empty(CAP, dtype=torch.int32, device="cuda:0")
    with pytest.raises(Exception):
        ctx.stage1_device(blanks.data_ptr(), 0xffffffc0, pos.data_ptr(), CAP)
    with pytest.raises(Exception):
        ctx.stage1_queue(blanks.data_ptr(), 0xffffffc0, pos.data_ptr(), CAP, 0)
    ctx.stage1_wait()


# ---- the message of a ticket, from the ticket ring ---------------------------------------------------------------------
RING_UNITS = [1, 1, 2, 33, 1, 32, 31, 1]  # T(j-1), T(j), T(j+1) belong to three messages in consecutive iterations


def spans(units, lead, body=None):
    """a message whose lead + len covers exactly `units` units"""
    size = units * UNIT - lead - 7
    return doc(size) if body is None else body + b" " * (size - len(body))


@pytest.mark.parametrize("lead", [0, 1, 63])
def test_message_resolution_from_the_ticket_ring(ctx, lead):
    """every message's count, verdict and positions against its own synchronous call and against the oracle (Msg.check)"""
    assert len(RING_UNITS) == G
    msgs = [Msg(spans(u, lead), lead=lead) for u in RING_UNITS]
    burst(ctx, msgs)
    burst(ctx, msgs[::-1])
    # an error and a short position buffer between clean neighbours
    msgs[4] = Msg(spans(1, lead, b'{"a":"\x01"}'), lead=lead)
    msgs[5] = Msg(spans(32, lead), lead=lead, cap=5)
    assert not msgs[4].ok_ref and msgs[3].ok_ref and msgs[6].ok_ref
    burst(ctx, msgs)
    ok, n, pos = msgs[5].single
    assert n == len(msgs[5].pos_ref) > 5 and len(pos) == 5


@pytest.mark.parametrize("nd", [False, True])
def test_blocks_cross_from_a_large_message_into_one_unit_messages(ctx, nd):
    """more than one round of tiles, then 1-unit messages: a block goes from the large message's last tiles into the small ones"""
    large = workloads.c2_twitter_array(60)
    assert len(large) > 257 * TILE
    msgs = [Msg(doc(UNIT - 9), nd=nd), Msg(large, nd=nd, lead=1)] + [Msg(doc(UNIT - 70 - k), nd=nd, lead=k) for k in (0, 1, 63, 5, 17, 40)]
    assert len(msgs) == G
    burst(ctx, msgs)
    ok, n, pos = msgs[1].single
    assert ok == msgs[1].ok_ref and (nd or (ok and n == workloads.c2_expected_structurals(60)))
