"""GPU tests of the grouped launches behind sjhip_stage1_device_queue (run with -m gpu on an MI355X): queued messages of one
mode run as one launch of the tile pipeline (stage1.hip GROUP), and nothing may cross the boundary between two of them.
Every message of a burst is checked against the oracle and against a single sjhip_stage1_device call on the same buffers."""
import os

import numpy as np
import pytest

import fixtures
import oracle_lib as O
import workloads

pytestmark = pytest.mark.gpu

G = 8             # messages per launch (sj_device.h S1_GROUP_MAX)
UNIT = 4096       # a wave unit
TILE = 32 * UNIT  # a full tile of the default kernel (1024 lanes x 2 passes x 64 bytes); a round is 256 tiles
GUARD = 64        # words behind every position buffer that nobody may write
SENTINEL = 0x5A5A5A5A


def test_the_environment_leaves_the_groups_on():
    """the A/B knobs of the library would turn every case below into single launches: a smaller group limit, or a kernel
    variant without a grouped form (stage1.hip stage1_group_limit)"""
    assert os.environ.get("SJHIP_S1_GROUP") is None and os.environ.get("SJHIP_S1_VARIANT") is None


@pytest.fixture(scope="module")
def ctx():
    import sjhip
    assert sjhip.supported(), "gfx950 device required"
    c = sjhip.Context(0)
    yield c
    c.close()


def doc(size):
    """a valid document of exactly `size` bytes with a structural at (nearly) every byte"""
    if size == 1:
        return b"7"
    m = (size - 1) // 2
    if m == 0:
        return b"[]"
    return b"[" + b" " * (size - 2 * m - 1) + b",".join([b"7"] * m) + b"]"


class Msg:
    """a message on the device at `lead` bytes behind a 64-byte boundary, its position buffer (cap words and GUARD sentinel
    words behind them) and what the oracle and a single launch say about it"""
    _oracle = {}

    def __init__(self, data, nd=False, lead=0, cap=None):
        import torch
        self.data, self.nd, self.lead = data, nd, lead
        key = (data, nd)
        if key not in Msg._oracle:
            Msg._oracle[key] = O.stage1(data, nd) if data else (False, np.zeros(0, np.uint32))
        self.ok_ref, self.pos_ref = Msg._oracle[key]
        self.cap = len(data) + 16 if cap is None else cap
        self.dev = torch.zeros(64 + len(data) + 256, dtype=torch.uint8, device="cuda:0")
        assert self.dev.data_ptr() % 64 == 0
        if data:
            self.dev[lead:lead + len(data)].copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
        self.pos = torch.empty(self.cap + GUARD, dtype=torch.int32, device="cuda:0")
        self.single = None

    def ptr(self):
        return self.dev.data_ptr() + self.lead

    def reset(self):
        self.pos.fill_(SENTINEL)

    def written(self, n):
        p = self.pos.cpu().numpy().view(np.uint32)
        assert np.all(p[self.cap:] == SENTINEL), "positions were written behind pos_cap"
        return p[:min(n, self.cap)].copy()

    def run_single(self, ctx):
        import torch
        if self.single is None:
            self.reset()
            torch.cuda.synchronize()
            ok, n = ctx.stage1_device(self.ptr(), len(self.data), self.pos.data_ptr(), self.cap, ndjson=self.nd)
            self.single = (ok, n, self.written(n))
        return self.single

    def check(self, ok, n, where):
        """(ok, n) and the positions in the buffer against the oracle and against the single launch"""
        got = self.written(n)
        s_ok, s_n, s_pos = self.single
        assert (ok, n) == (s_ok, s_n), (where, ok, n, s_ok, s_n)
        assert np.array_equal(got, s_pos), where
        if not self.data:
            assert (ok, n) == (False, 0), where
            return
        assert ok == self.ok_ref, where
        if self.ok_ref:
            assert n == len(self.pos_ref), where
            assert np.array_equal(got, self.pos_ref[:self.cap]), where


def burst(ctx, msgs, between=None):
    """queues msgs in one burst (slot = index), waits once and checks every message; between: (index, callable) run
    in front of that message's _queue call"""
    import torch
    for m in msgs:
        m.run_single(ctx)
    for m in msgs:
        m.reset()
    torch.cuda.synchronize()
    for slot, m in enumerate(msgs):
        if between and between[0] == slot:
            between[1]()
        ctx.stage1_queue(m.ptr(), len(m.data), m.pos.data_ptr(), m.cap, slot, ndjson=m.nd)
    ctx.stage1_wait()
    for slot, m in enumerate(msgs):
        ok, n = ctx.stage1_result(slot, len(m.data))
        m.check(ok, n, (slot, len(m.data), m.lead))


SEAM_SIZES = [1, UNIT - 1, UNIT, UNIT + 1, TILE - UNIT, TILE, TILE + 1, 3 * TILE + 1000]


@pytest.mark.parametrize("lead", [0, 1, 31, 63])
def test_tile_plan_seams_inside_a_group(ctx, lead):
    """one group of G messages whose sizes sit on the seams of the tile plan, in this order and reversed"""
    assert len(SEAM_SIZES) == G
    msgs = [Msg(doc(s), lead=lead) for s in SEAM_SIZES]
    burst(ctx, msgs)
    burst(ctx, msgs[::-1])


def test_no_state_crosses_a_message_boundary(ctx):
    """A ends inside a string / on an odd run of backslashes inside a string / on a structural; B's first byte would read
    differently with A's end state: B's verdict, count and positions are those of B alone"""
    pairs = [(b'{"open":"never closed', b'"x":1}'),
             (b'{"k":"abc\\\\\\', b'"}'),
             (b'{"a":[1,2]}', b'12345'),
             (b'{"a":[1,2],', b'true')]
    msgs = [Msg(d) for pair in pairs for d in pair]
    assert len(msgs) == G
    burst(ctx, msgs)
    burst(ctx, msgs[::-1])


def test_errors_stay_with_their_message(ctx):
    tw = fixtures.load("twitter")
    bad = b'{"a":"' + b"x" * 5000 + b"\x01" + b"y" * 5000 + b'"}'
    msgs = [Msg(tw), Msg(bad), Msg(tw * 2), Msg(b'{"a":"\x01"}'), Msg(doc(TILE + 1))]
    assert not msgs[1].ok_ref and not msgs[3].ok_ref and msgs[0].ok_ref and msgs[2].ok_ref and msgs[4].ok_ref
    burst(ctx, msgs)


def test_a_short_position_buffer_between_two_with_room(ctx):
    """the message in the middle takes the path without room (fits == false): what fits is written, its count is the whole
    count, its neighbours are exact and nobody writes behind a pos_cap (the sentinel words behind every buffer)"""
    big = doc(2 * TILE + 777)
    for cap in (0, 5, 4095, TILE + 3):
        msgs = [Msg(doc(TILE + 1)), Msg(big, cap=cap), Msg(doc(3 * UNIT))]
        burst(ctx, msgs)
        ok, n, pos = msgs[1].single
        assert n == len(msgs[1].pos_ref) > cap and len(pos) == cap


def test_group_boundaries(ctx):
    """2 G + 3 messages in one burst: several groups and a short last one; an ND message and an empty one in the middle; a
    synchronous launch on the same context between two _queue calls; the slots are used again in a second burst"""
    import torch
    tw = fixtures.load("twitter")
    nd = workloads.c5_parking_nd(40).rstrip(b"\n")
    msgs = [Msg(doc(1000 + 37 * k), lead=k % 64) for k in range(2 * G + 3)]
    msgs[5] = Msg(nd, nd=True)
    msgs[6] = Msg(nd, nd=True, lead=3)
    msgs[11] = Msg(b"")
    msgs[13] = Msg(tw)
    assert msgs[5].ok_ref
    side = Msg(tw * 3)
    side.run_single(ctx)

    def sync_call():
        side.reset()
        torch.cuda.synchronize()
        ok, n = ctx.stage1_device(side.ptr(), len(side.data), side.pos.data_ptr(), side.cap)
        side.check(ok, n, "synchronous call between two queued ones")

    for k in (3, 9):
        burst(ctx, msgs, between=(k, sync_call))
    burst(ctx, msgs[::-1])


def test_result_needs_a_wait(ctx):
    """a queued message starts no later than the next _wait; until then its slot has no result"""
    m = Msg(doc(5000))
    m.run_single(ctx)
    m.reset()
    ctx.stage1_queue(m.ptr(), len(m.data), m.pos.data_ptr(), m.cap, 7)
    with pytest.raises(Exception, match="left no result"):
        ctx.stage1_result(7, len(m.data))
    ctx.stage1_wait()
    ok, n = ctx.stage1_result(7, len(m.data))
    m.check(ok, n, "after _wait")


def test_blocks_wrap_across_messages(ctx):
    """small / more than one round of tiles / small in one group: the blocks draw the large message's tiles, wrap around
    and go on into the last message"""
    large = workloads.c2_twitter_array(60)
    assert len(large) > 257 * TILE
    msgs = [Msg(doc(3 * UNIT + 5), lead=31), Msg(large, lead=1), Msg(doc(TILE + UNIT + 9), lead=63)]
    burst(ctx, msgs)
    ok, n, pos = msgs[1].single
    assert ok and n == workloads.c2_expected_structurals(60)
