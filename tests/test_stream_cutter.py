"""CPU: the block cutter of ParseNDStream (sjhip/stream.py read_block / cut_blocks) against a serial restatement of the
reference's loop (simdjson_amd64.go:155-176, with its Read taken as a full read: short reads are not the end), on
readers that deliver a few bytes at a time, at block sizes down to one byte and at every kind of line end."""
import io
import random

import pytest

from sjhip.stream import cut_blocks, read_block

BLOCK_SIZES = [1, 2, 7, 64, 4096]


def go_loop(data, block_size):
    """The reference's reader goroutine, one statement per step (:155-176): fill tmp, and unless the input ended inside it
    append up to and including the next newline; a block that is empty is not queued; the end of the input ends the loop."""
    pos, blocks = 0, []
    while True:
        tmp = data[pos:pos + block_size]                      # :158  n, err := buf.Read(tmp)
        pos += len(tmp)
        eof = len(tmp) < block_size
        if not eof:                                           # :165  if err != io.EOF
            nl = data.find(b"\n", pos)                        # :166  b, err2 := buf.ReadBytes('\n')
            end = len(data) if nl < 0 else nl + 1
            tmp, pos, eof = tmp + data[pos:end], end, nl < 0  # :171, :173
        if tmp:                                               # :176  if len(tmp) > 0
            blocks.append(tmp)
        if eof:                                               # :209
            return blocks


class Trickle(io.RawIOBase):
    """a raw reader that hands out 1 to 7 bytes per readinto"""

    def __init__(self, data, seed=0):
        self.d, self.p, self.rnd = data, 0, random.Random(seed)

    def readable(self):
        return True

    def readinto(self, b):
        n = min(len(b), self.rnd.randrange(1, 8), len(self.d) - self.p)
        b[:n] = self.d[self.p:self.p + n]
        self.p += n
        return n


class NoReadline:
    """a reader with readinto (short reads) and nothing else: cut_blocks has to buffer it to find line ends"""

    def __init__(self, data, seed=0):
        self._raw = Trickle(data, seed)
        self.closed = False

    def readable(self):
        return True

    def readinto(self, b):
        return self._raw.readinto(b)

    def close(self):
        self.closed = True


class ShortReadsWithReadline:
    """a reader that has readline and whose readinto is short: used as it is, so read_block's own loop has to fill the block"""

    def __init__(self, data, seed=0):
        self._b, self.rnd = io.BytesIO(data), random.Random(seed)

    def readinto(self, b):
        return self._b.readinto(memoryview(b)[:self.rnd.randrange(1, 8)])

    def readline(self):
        return self._b.readline()


READERS = [io.BytesIO, Trickle, NoReadline, ShortReadsWithReadline]


def _inputs():
    rnd = random.Random(8)
    lines = [b"x" * rnd.randrange(0, 40) for _ in range(60)]
    yield "no newline at the end", b"\n".join(lines)
    yield "newline at the end", b"\n".join(lines) + b"\n"
    for bs in BLOCK_SIZES:  # every line ends exactly where a block is full, and a few of them one byte off
        if bs <= 64:
            yield f"lines of {bs} bytes", (b"y" * (bs - 1) + b"\n") * 9
            yield f"lines of {bs} and {bs + 1} bytes", (b"y" * (bs - 1) + b"\n" + b"z" * bs + b"\n") * 5 + b"tail"
    yield "4096-byte lines", (b"y" * 4095 + b"\n") * 3
    yield "a line longer than several blocks", b"ab\n" + b"L" * 9000 + b"\ncd\n" + b"M" * 300
    yield "crlf", b"\r\n".join(lines[:30]) + b"\r\n"
    yield "blank lines only", b"\n" * 150
    yield "blank lines, crlf", b"\r\n" * 70
    yield "one byte", b"x"
    yield "one newline", b"\n"
    yield "empty", b""


INPUTS = list(_inputs())


@pytest.mark.parametrize("block_size", BLOCK_SIZES)
@pytest.mark.parametrize("make_reader", READERS, ids=[r.__name__ for r in READERS])
def test_cut_blocks_is_the_reference_loop(make_reader, block_size):
    for name, data in INPUTS:
        blocks = list(cut_blocks(make_reader(data), block_size))
        what = (name, block_size)
        assert b"".join(blocks) == data, what
        assert all(len(b) >= block_size and b.endswith(b"\n") for b in blocks[:-1]), what
        assert all(len(b) > 0 for b in blocks), what
        assert blocks == go_loop(data, block_size), what
    assert list(cut_blocks(make_reader(b""), block_size)) == []


@pytest.mark.parametrize("make_reader", READERS, ids=[r.__name__ for r in READERS])
def test_block_full_at_a_line_end_takes_the_next_line_too(make_reader):
    """Expected, because it is what the reference does: ReadBytes('\\n') runs whenever the block was filled, also when its
    last byte is a newline, and then returns the whole next line.  So blocks that are full exactly at a line end are one
    line longer than the block size asks for, and the last line of the input never gets a block of its own that way."""
    data = b"aaa\nbbb\ncc\nd\n\neeeeeee\nf"
    assert list(cut_blocks(make_reader(data), 4)) == [b"aaa\nbbb\n", b"cc\nd\n", b"\neeeeeee\n", b"f"]
    assert list(cut_blocks(make_reader(b"aaa\nbbb\n"), 4)) == [b"aaa\nbbb\n"]
    assert list(cut_blocks(make_reader(b"aaa\n"), 4)) == [b"aaa\n"]          # full, and nothing follows
    assert list(cut_blocks(make_reader(b"aaa\nb"), 4)) == [b"aaa\nb"]        # the rest of the input has no newline
    assert list(cut_blocks(make_reader(b"aaa\n\n\n"), 4)) == [b"aaa\n\n", b"\n"]
    for d in (data, b"aaa\nbbb\n", b"aaa\n", b"aaa\nb", b"aaa\n\n\n"):
        assert list(cut_blocks(make_reader(d), 4)) == go_loop(d, 4)


def test_read_block_returns_the_tail_apart():
    """read_block: at most block_size bytes into the view; the rest of the line comes back separately (the stream copies
    it behind the block, after growing the pinned block if it has to)"""
    for make_reader in (io.BytesIO, ShortReadsWithReadline):
        r = make_reader(b"0123456789\nabc\n")
        view = memoryview(bytearray(8))
        assert read_block(r, view, 8) == (8, b"89\n") and bytes(view) == b"01234567"
        assert read_block(r, view, 8) == (4, b"") and bytes(view[:4]) == b"abc\n"
        assert read_block(r, view, 8) == (0, b"")
        r = make_reader(b"0123456\n")
        assert read_block(r, view, 8) == (8, b"") and read_block(r, view, 8) == (0, b"")
        # a view larger than the block (the stream's pinned block has a reserve): only block_size bytes are read into it
        r = make_reader(b"0123456789\n")
        big = memoryview(bytearray(b"." * 16))
        assert read_block(r, big, 4) == (4, b"456789\n") and bytes(big) == b"0123" + b"." * 12
