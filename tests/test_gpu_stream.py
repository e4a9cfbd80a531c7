"""GPU: the states of sjhip_stream_* (csrc/stream_api.hip) and of sjhip/stream.py on top of it, on small blocks: the call
contract of include/sjhip.h code by code, slots reused for results of very different sizes, the filtered stream at the
edges of a block, where the first error falls, and one thread submitting while another takes results.

The arbiter is the oracle's ParseND (copied strings) of every block as sjhip.cut_blocks cuts it; for a filtered stream, of
the block's matching lines.  The ring, the pinned buffers and the ordering do not depend on the block size, so the blocks
are 4 KiB to 64 KiB.  Every wait on a stream goes through stream_util.bounded: a lost wake-up fails, it does not hang."""
import ctypes as C
import io
import queue
import threading
import time

import numpy as np
import pytest

import stream_util as U
from stream_util import CLOSED, EMPTY, ERR_ARG, ERR_STAGE1, ERR_STAGE2, FULL, OK

pytestmark = pytest.mark.gpu

BS = 4096
DOC = b'{"a":1}\n{"b":"xy","c":[1,2.5,null]}\n'   # a short block
DOC2 = b'{"k":"v"}\n{"k":"w"}\n{"z":true}\n'


@pytest.fixture(scope="module", autouse=True)
def _device():
    import sjhip
    assert sjhip.supported(), "gfx950 device required"
    yield
    print(f"\nslowest bounded call: {U.SLOWEST[0]:.3f} s ({U.SLOWEST[1]})")


# ---- a. the call contract ------------------------------------------------------------------------------------------------------
def test_fresh_stream():
    with U.Raw(BS, 2) as s:
        assert s.slots() == 2 and s.block_capacity() == BS
        rc, _ = s.next()
        assert rc == EMPTY
        assert s.ready() == 0 and s.in_flight() == 0
        assert s.release() == ERR_ARG and s.cancel() == ERR_ARG and s.submit(0) == ERR_ARG
        assert s.grow(0, 2 * BS)[0] == ERR_ARG
        # none of the refused calls changed anything: the stream still parses
        assert s.submit_copy(DOC) == OK
        rc, got, _ = s.take()
        assert rc == OK
        U.assert_block(got, DOC)
    with U.Raw(BS, 0) as s:  # slots = 0: three per device
        assert s.slots() == 3 and s.block_capacity() == BS
    with U.Raw(BS, 5) as s:
        assert s.slots() == 5


def test_acquire_twice_cancel_and_submit_too_long():
    with U.Raw(BS, 2) as s:
        rc, p0, cap = s.acquire()
        assert rc == OK and p0 and cap == BS
        rc, _, _ = s.acquire()
        assert rc == ERR_ARG and "already acquired" in s.last_error()
        # the first block is still the acquired one: cancel hands it back, and the same slot's block comes again
        assert s.cancel() == OK and s.cancel() == ERR_ARG
        rc, p1, cap = s.acquire()
        assert rc == OK and p1 == p0 and cap == BS
        # a submit that is too long is refused and leaves the block acquired
        C.memmove(p1, DOC, len(DOC))
        assert s.submit(cap + 1) == ERR_ARG and s.in_flight() == 0
        assert s.acquire()[0] == ERR_ARG          # (still acquired)
        assert s.submit(len(DOC)) == OK and s.in_flight() == 1
        assert s.submit(len(DOC)) == ERR_ARG      # (and now it is not)
        rc, got, _ = s.take()
        assert rc == OK
        U.assert_block(got, DOC)
        # the next acquire moves on to the other slot
        rc, p2, _ = s.acquire()
        assert rc == OK and p2 != p0
        assert s.cancel() == OK


@pytest.mark.parametrize("S", [1, 2, 3, 5])
def test_full_ring_next_release(S):
    blocks = [b'{"i":%d,"s":"%s"}\n' % (i, b"q" * (i * 37)) for i in range(S + 1)]
    with U.Raw(BS, S) as s:
        for blk in blocks[:S]:
            assert s.submit_copy(blk) == OK
        assert s.acquire()[0] == FULL and s.submit_copy(blocks[S]) == FULL
        assert s.in_flight() == S
        s.wait_ready()                      # ready becomes 1 ...
        t0 = time.perf_counter()
        rc, r = s.next()                    # ... and next then returns at once (it only takes the stream's mutex)
        assert rc == OK and time.perf_counter() - t0 < 1.0
        U.assert_block(U.copy_result(r), blocks[0])
        assert s.in_flight() == S - 1
        # a result is held: no second one, and ready says so
        rc2, r2 = s.next()
        assert rc2 == ERR_ARG and "not been released" in s.last_error() and r2.tape_len == 0 and not r2.tape
        assert s.ready() == 0
        assert s.acquire()[0] == FULL       # the held block's slot is not free yet
        U.assert_block(U.copy_result(r), blocks[0])  # the refused calls left the held result alone
        assert s.release() == OK and s.release() == ERR_ARG
        assert s.submit_copy(blocks[S]) == OK
        for blk in blocks[1:]:
            rc, got, _ = s.take()
            assert rc == OK
            U.assert_block(got, blk)
        assert s.next()[0] == EMPTY and s.in_flight() == 0


def test_set_filter_states():
    with U.Raw(BS, 1) as s:   # one slot: every block meets what the one before it left there
        rc, ptr, _ = s.acquire()
        assert rc == OK
        assert s.set_filter(b"k", b"v") == ERR_ARG and "in flight" in s.last_error()    # a block is acquired
        C.memmove(ptr, DOC2, len(DOC2))
        assert s.submit(len(DOC2)) == OK
        assert s.set_filter(b"k", b"v") == ERR_ARG                                      # a block is in flight
        rc, r = s.next()
        assert rc == OK and s.set_filter(b"k", b"v") == OK                              # delivered: nothing is in flight
        got = U.copy_result(r)
        assert s.release() == OK
        U.assert_block(got, DOC2, "the refused set_filter left the stream unfiltered")
        assert r.records == 0
        assert s.submit_copy(DOC2) == OK
        rc, got, records = s.take()
        assert rc == OK
        U.assert_filtered(got[:2], records, DOC2, "k", "v")
        assert records == 1
        assert s.set_filter(b"", b"") == OK                                             # klen = 0: off again
        assert s.submit_copy(DOC2) == OK
        rc, got, records = s.take()
        assert rc == OK and records == 0
        U.assert_block(got, DOC2, "filter turned off")


def _exactly(n):
    """an NDJSON block of exactly n bytes"""
    head = b'{"a":1}\n{"b":[true,false]}\n'
    return head + b'{"pad":"' + b"p" * (n - len(head) - 11) + b'"}\n'


@pytest.mark.parametrize("S", [1, 3])
def test_submit_copy_sizes(S):
    big = U.fill(U.long_string_lines(), 3 * BS)        # larger than the capacity: the grow path with keep = 0
    exact = _exactly(BS)
    assert len(big) > 3 * BS and len(exact) == BS
    blocks = [DOC, big, exact, DOC2] * 2 + [big, DOC]
    with U.Raw(BS, S) as s:
        got, rc = U.run_raw(s, blocks)
        assert rc == EMPTY and len(got) == len(blocks)
        for i, (res, blk) in enumerate(zip(got, blocks)):
            U.assert_block(res, blk, i)
        assert s.block_capacity() == BS   # (what create was asked for; a slot that has grown says so in acquire)
        # a block of length 0 is parsed like any other: the oracle's verdict on an empty document, which ends the stream
        ref = U.oracle(b"")
        assert ref.rc != 0
        assert s.submit_copy(DOC) == OK and s.submit_copy(b"") == (OK if S > 1 else FULL)
        rc, res, _ = s.take()
        assert rc == OK
        U.assert_block(res, DOC)
        if S == 1:
            assert s.submit_copy(b"") == OK
        assert s.in_flight() == 1
        rc, r = s.next()
        assert rc == ref.rc and r.tape_len == 0
        assert s.next()[0] == CLOSED and s.acquire()[0] == CLOSED and s.submit_copy(DOC) == CLOSED
        assert s.in_flight() == 0 and s.ready() == 1


@pytest.mark.parametrize("S", [1, 2, 3])
def test_grow_keeps_bytes_and_capacity(S):
    keep = 1000
    head = bytes((7 * i + 3) & 0xff for i in range(keep))
    with U.Raw(BS, S) as s:
        rc, p0, cap = s.acquire()
        assert rc == OK and cap == BS
        C.memmove(p0, head, keep)
        for smaller in (BS, BS - 1, 1, 0):                 # no larger than the current one: the same block
            assert s.grow(keep, smaller) == (OK, p0)
        rc, p1 = s.grow(keep, 3 * BS)
        assert rc == OK and p1 and C.string_at(p1, keep) == head
        assert s.grow(keep, 3 * BS) == (OK, p1) and s.grow(0, 2 * BS) == (OK, p1)
        # the grown capacity is the slot's: a submit up to it is accepted, one past it is not
        long_block = U.fill(U.long_string_lines(3), 2 * BS + 500)
        assert BS < len(long_block) <= 3 * BS
        C.memmove(p1, long_block, len(long_block))
        assert s.submit(3 * BS + 1) == ERR_ARG
        assert s.submit(len(long_block)) == OK
        rc, got, _ = s.take()
        assert rc == OK
        U.assert_block(got, long_block)
        # the other slots still have the capacity of create; S submissions later the grown one comes round again
        for k in range(1, S):
            rc, p, cap = s.acquire()
            assert rc == OK and cap == BS and p != p1
            C.memmove(p, DOC, len(DOC))
            assert s.submit(len(DOC)) == OK
            rc, got, _ = s.take()
            assert rc == OK
            U.assert_block(got, DOC)
        rc, p, cap = s.acquire()
        assert rc == OK and p == p1 and cap == 3 * BS
        assert s.block_capacity() == BS
        C.memmove(p, DOC2, len(DOC2))                      # a short block in the grown slot
        assert s.submit(len(DOC2)) == OK
        rc, got, _ = s.take()
        assert rc == OK
        U.assert_block(got, DOC2)


# ---- b. slots reused for results of very different sizes ---------------------------------------------------------------------
# D: many tiny records (large tape, little Strings.B); L: few records with long strings (small tape, large Strings.B);
# B: a single record just over the block size.  59 blocks of this period-11 pattern: 59 is coprime to every slot count,
# and with it every slot of every S in (1, 2, 3, 5) sees every kind directly after every other kind (asserted below).
PATTERN = "DDDBLDLBLLB"
N_BLOCKS = 59
SLOTS = (1, 2, 3, 5)


def _reuse_input():
    dense, longs = U.dense_lines(), U.long_string_lines()
    kinds = (PATTERN * 6)[:N_BLOCKS]
    segs = [U.fill(dense, BS) if k == "D" else U.fill(longs, BS) if k == "L" else U.one_record(BS, 100 + 8 * i)
            for i, k in enumerate(kinds)]
    return kinds, segs


_REUSE = []


def reuse_blocks():
    """-> (kinds, blocks): built, cut and checked once"""
    import sjhip
    if not _REUSE:
        kinds, segs = _reuse_input()
        blocks = list(sjhip.cut_blocks(io.BytesIO(b"".join(segs)), BS))
        assert blocks == segs, "the cutter does not cut where the input was built to be cut"
        pairs = {(a, b) for a in "DLB" for b in "DLB" if a != b}
        for S in SLOTS:
            for slot in range(S):
                mine = kinds[slot::S]
                assert pairs <= set(zip(mine, mine[1:])), (S, slot)
        tl = [len(U.oracle(b).tape) for b in blocks]
        sl = [len(U.oracle(b).strings) for b in blocks]
        assert max(tl) > 10 * min(tl) and max(sl) > 10 * min(sl), (max(tl), min(tl), max(sl), min(sl))
        _REUSE.append((kinds, blocks))
    return _REUSE[0]


@pytest.mark.parametrize("view", [False, True])
@pytest.mark.parametrize("S", SLOTS)
def test_slot_reuse_sizes(S, view):
    import sjhip
    _, blocks = reuse_blocks()
    got = U.drain(sjhip.parse_nd_stream(io.BytesIO(b"".join(blocks)), block_size=BS, inflight=S, view=view))
    assert len(got) == len(blocks)
    for i, (res, blk) in enumerate(zip(got, blocks)):
        U.assert_block(res[:3], blk, (S, view, i))
        assert res[3] == 0


@pytest.mark.parametrize("S", SLOTS)
def test_slot_reuse_with_recycled_results(S):
    """`reuse`: every delivered ParsedJson goes back, so its buffers are larger than some next results and smaller than others"""
    import sjhip
    _, blocks = reuse_blocks()
    back = queue.SimpleQueue()
    caps = []

    def give_back(pj):
        caps.append((pj._tape_buf.size, pj._str_buf.size))
        back.put(pj)

    got = U.drain(sjhip.parse_nd_stream(io.BytesIO(b"".join(blocks)), block_size=BS, inflight=S, reuse=back), after=give_back)
    assert len(got) == len(blocks)
    for i, (res, blk) in enumerate(zip(got, blocks)):
        U.assert_block(res[:3], blk, (S, i))
    # a recycled buffer was kept where it was large enough (capacity above the result's size) and replaced where not
    sizes = [(len(U.oracle(b).tape), len(U.oracle(b).strings)) for b in blocks]
    assert any(c[0] > n[0] for c, n in zip(caps, sizes)) and any(c[1] > n[1] for c, n in zip(caps, sizes))
    assert all(c[0] >= n[0] and c[1] >= n[1] for c, n in zip(caps, sizes))


@pytest.mark.parametrize("S", SLOTS)
def test_block_counts_around_the_ring(S):
    """S-1, S, S+1 and 2S+1 blocks, cut from a prefix of the same input"""
    import sjhip
    _, blocks = reuse_blocks()
    for n in (S - 1, S, S + 1, 2 * S + 1):
        for view in (False, True):
            prefix = b"".join(blocks[:n])
            assert list(sjhip.cut_blocks(io.BytesIO(prefix), BS)) == blocks[:n]
            got = U.drain(sjhip.parse_nd_stream(io.BytesIO(prefix), block_size=BS, inflight=S, view=view))
            assert len(got) == n, (S, n, view, len(got))
            for i, (res, blk) in enumerate(zip(got, blocks)):
                U.assert_block(res[:3], blk, (S, n, view, i))


# ---- c. the filtered stream at the edges of a block -----------------------------------------------------------------------------
KEY, VALUE = "Make", "HOND"
FILTER_KINDS = ["all", "none", "all", "all", "none", "first", "none", "last", "all", "all", "other", "none", "all", "none"]


def _hit(i):
    return b'{"Ticket":%d,"Make":"HOND","Color":"%s"}' % (4270000000 + i, b"WH" * (1 + i % 5))


def _misses():
    """lines that hold the wanted bytes and do not match"""
    i = 0
    shapes = [b'{"Ticket":%d,"Make":7,"Note":"HOND"}',                     # the key holds a non-string
              b'{"Ticket":%d,"Car":{"Make":"HOND"},"Note":"Make"}',        # the key one level down
              b'{"Ticket":%d,"Make":"HON"}',                               # a proper prefix of the value
              b'{"Ticket":%d,"Make":"HONDA"}',                             # a proper extension of it
              b'{"Ticket":%d,"Make":null,"Body":["Make","HOND"]}',
              b'{"Ticket":%d,"make":"HOND","Make ":"HOND","Mak":"HOND"}',
              b'{"Ticket":%d,"Make":"TOYT","Color":"HOND"}']
    while True:
        yield shapes[i % len(shapes)] % i
        i += 1


def _filter_segment(kind, n_lines, seed):
    miss = _misses()
    for _ in range(seed):
        next(miss)
    lines = []
    for j in range(n_lines):
        hit = {"all": True, "none": False, "first": j == 0, "last": j == n_lines - 1, "other": j % 2 == 0}[kind]
        lines.append(_hit(seed + j) if hit else next(miss))
    return lines


_FILTER = []


def filter_blocks():
    import sjhip
    if not _FILTER:
        segs = []
        for i, kind in enumerate(FILTER_KINDS):
            n = 1
            while sum(len(ln) + 1 for ln in _filter_segment(kind, n, 3 * i)) <= BS:  # as U.fill: just past the block size
                n += 1
            segs.append(b"".join(ln + b"\n" for ln in _filter_segment(kind, n, 3 * i)))
        blocks = list(sjhip.cut_blocks(io.BytesIO(b"".join(segs)), BS))
        assert blocks == segs
        for blk, kind in zip(blocks, FILTER_KINDS):
            lines = blk.split(b"\n")[:-1]
            want = U.matching_lines(blk, KEY, VALUE)
            assert want == {"all": lines, "none": [], "first": lines[:1], "last": lines[-1:], "other": lines[::2]}[kind], kind
            assert kind == "all" or sum(b'"HOND"' in ln for ln in lines) > len(want)  # a substring search would be fooled
        for S in (1, 3):  # an empty result follows a full one on the same slot, and the reverse
            after = set(zip(FILTER_KINDS, FILTER_KINDS[S:]))
            assert ("all", "none") in after and ("none", "all") in after, S
        _FILTER.append(blocks)
    return _FILTER[0]


@pytest.mark.parametrize("view", [False, True])
@pytest.mark.parametrize("S", [1, 3])
def test_filtered_stream_block_edges(S, view):
    import sjhip
    blocks = filter_blocks()
    it = sjhip.parse_nd_stream(io.BytesIO(b"".join(blocks)), block_size=BS, inflight=S, view=view, where=(KEY.encode(), VALUE.encode()))
    got = U.drain(it)
    assert len(got) == len(blocks)
    for i, (res, blk) in enumerate(zip(got, blocks)):
        U.assert_filtered(res[:2], res[3], blk, KEY, VALUE, (S, view, i, FILTER_KINDS[i]))


# ---- d. where the first error falls ------------------------------------------------------------------------------------------
def _error_blocks(n, bad, big=None):
    """n blocks of alternating kinds; bad = {position: bad line}: that block holds the line, in the middle of good ones;
    `big`: the position of a block with one long record (the largest block of the stream by far)"""
    dense, longs = U.dense_lines(5), U.long_string_lines(5, 900)
    segs = []
    for i in range(n):
        first = [next(dense), bad[i], next(dense)] if i in bad else []
        if i == big:
            first.append(b'{"big":"' + b"z" * (60 << 10) + b'"}')
        segs.append(U.fill(longs if i & 1 else dense, BS, first))
    return segs


def _after_the_error(s):
    assert s.next()[0] == CLOSED
    assert s.acquire()[0] == CLOSED
    assert s.in_flight() == 0
    assert s.ready() == 1
    assert s.next()[0] == CLOSED and s.submit_copy(DOC) == CLOSED
    s.destroy()  # (under the bound)


@pytest.mark.parametrize("bad_line", [U.BAD_STAGE1, U.BAD_STAGE2], ids=["stage1", "stage2"])
@pytest.mark.parametrize("S", [1, 2, 3])
def test_first_error_at_every_position(S, bad_line):
    import sjhip
    n = 2 * S + 2
    for p in range(n):
        blocks = _error_blocks(n, {p: bad_line})
        data = b"".join(blocks)
        assert list(sjhip.cut_blocks(io.BytesIO(data), BS)) == blocks
        ref = U.oracle(blocks[p])
        assert ref.rc == (ERR_STAGE1 if bad_line is U.BAD_STAGE1 else ERR_STAGE2)
        # the C API
        with U.Raw(BS, S) as s:
            got, rc = U.run_raw(s, blocks)
            assert rc == ref.rc and len(got) == p, (S, p, rc, len(got))
            for i, res in enumerate(got):
                U.assert_block(res, blocks[i], (S, p, i))
            _after_the_error(s)
        # the generator
        with pytest.raises(sjhip.ParseError) as e:
            U.drain(sjhip.parse_nd_stream(io.BytesIO(data), block_size=BS, inflight=S))
        assert e.value.code == ref.rc and len(e.value.delivered) == p, (S, p, e.value.code, len(e.value.delivered))
        for i, res in enumerate(e.value.delivered):
            U.assert_block(res[:3], blocks[i], (S, p, i))


@pytest.mark.parametrize("S", [2, 3])
def test_two_bad_blocks_the_earlier_one_wins(S):
    """the earlier bad block is the largest of the stream and the later one is tiny, so the later one tends to finish first"""
    n = 2 * S + 2
    for p in range(n):
        for q in range(p + 1, min(p + S - 1, n - 1) + 1):
            for first, second in ((U.BAD_STAGE2, U.BAD_STAGE1), (U.BAD_STAGE1, U.BAD_STAGE2)):
                blocks = _error_blocks(n, {p: first}, big=p)
                blocks[q] = second + b"\n"
                assert len(blocks[p]) == max(map(len, blocks)) and len(blocks[q]) == min(map(len, blocks))
                want = U.oracle(blocks[p]).rc
                assert want not in (0, U.oracle(blocks[q]).rc) and U.oracle(blocks[q]).rc != 0
                with U.Raw(BS, S) as s:
                    got, rc = U.run_raw(s, blocks)
                    assert rc == want and len(got) == p, (S, p, q, rc, want, len(got))
                    for i, res in enumerate(got):
                        U.assert_block(res, blocks[i], (S, p, q, i))
                    _after_the_error(s)


@pytest.mark.parametrize("S", [1, 2, 3, 5])
def test_close_with_blocks_queued_and_a_result_held(S):
    import sjhip
    _, blocks = reuse_blocks()
    it = sjhip.parse_nd_stream(io.BytesIO(b"".join(blocks)), block_size=BS, inflight=S, view=True)
    pj = U.bounded(next, it)          # the ring was filled before this result was taken: it is held, the rest is queued
    U.assert_block((pj.Tape, pj.Strings, pj.Message), blocks[0])
    U.bounded(it.close)
    # the same on the C API, where the numbers can be seen
    with U.Raw(BS, S) as s:
        for blk in blocks[:S]:
            assert s.submit_copy(blk) == OK
        rc, r = s.next()
        assert rc == OK and s.in_flight() == S - 1
        s.destroy()


# ---- e. one thread submits while another takes results -----------------------------------------------------------------------
def test_one_thread_feeds_another_takes():
    import sjhip
    from sjhip.stream import Stream
    dense, longs = U.dense_lines(), U.long_string_lines(0, 700)
    segs = [U.fill(longs if i % 3 == 1 else dense, BS) for i in range(160)]
    data = b"".join(segs)
    assert list(sjhip.cut_blocks(io.BytesIO(data), BS)) == segs
    st = Stream(BS, slots=3)
    reader = io.BytesIO(data)
    fed, got, errors = threading.Event(), [], []

    def produce():
        try:
            while True:
                state = st.feed(reader)
                if state == "full":
                    time.sleep(0.0002)
                elif state != "more":
                    return
        except BaseException as e:  # noqa: BLE001
            errors.append(e)
        finally:
            fed.set()

    def consume():
        try:
            while True:
                done = fed.is_set()  # (read before the take: nothing is submitted after it is set)
                pj = st.take()
                if pj is not None:
                    got.append((pj.Tape, pj.Strings, pj.Message))
                elif done:
                    return
                else:
                    time.sleep(0.0002)
        except BaseException as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=f, daemon=True) for f in (produce, consume)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(U.JOIN_S)
    assert not any(t.is_alive() for t in threads), "producer or consumer still running: a lost wake-up?"
    assert not errors, errors
    assert len(got) == len(segs) and st.in_flight() == 0
    for i, (res, blk) in enumerate(zip(got, segs)):
        U.assert_block(res, blk, i)
    U.bounded(st.close)
