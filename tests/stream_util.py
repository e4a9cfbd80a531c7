"""Shared pieces of tests/test_gpu_stream.py: the bounded wait, the raw sjhip_stream_* calls through ctypes, inputs whose
blocks the cutter cuts exactly where the test wants them, and the oracle's verdict on a block (computed once per block).
Nothing here needs a GPU to be imported."""
import ctypes as C
import json
import threading
import time

import numpy as np

import oracle_lib as O

OK, ERR_STAGE1, ERR_STAGE2, ERR_ARG, FULL, EMPTY, CLOSED = 0, 1, 2, 5, 6, 7, 8  # include/sjhip.h

# Every wait on a stream runs on a daemon thread that is joined with this bound, so a lost wake-up is a failed assertion
# and not a hung test.  The slowest bounded call is the first step of a generator: it creates the stream (contexts, pinned
# blocks, worker threads) and parses the first block on a context that has not run a kernel yet.  Slowest observed:
# NOT YET MEASURED on the device (0.08 s with the parse replaced by the CPU oracle); test_gpu_stream.py prints the figure
# of a run at the end of the module (pytest -s).
JOIN_S = 30.0
SLOWEST = [0.0, ""]  # the slowest bounded call of the process so far: (seconds, what)


def bounded(fn, *args, **kw):
    """fn(*args, **kw) on a daemon thread; fails if it has not returned after JOIN_S.  -> its value (or raises what it raised)"""
    box = {}

    def run():
        try:
            box["v"] = fn(*args, **kw)
        except BaseException as e:  # noqa: BLE001 -- handed to the caller below
            box["e"] = e

    t = threading.Thread(target=run, daemon=True)
    t0 = time.perf_counter()
    t.start()
    t.join(JOIN_S)
    what = getattr(fn, "__name__", repr(fn))
    assert not t.is_alive(), f"{what} has not returned after {JOIN_S} s: a lost wake-up?"
    dt = time.perf_counter() - t0
    if dt > SLOWEST[0]:
        SLOWEST[:] = [dt, what]
    if "e" in box:
        raise box["e"]
    return box.get("v")


# ---- the oracle's verdict on a block, and on the matching lines of a block --------------------------------------------------
_REF = {}


def oracle(blk):
    """oracle_lib.parse(blk, ndjson=True, copy_strings=True), computed once per distinct block and never modified"""
    blk = bytes(blk)
    ref = _REF.get(blk)
    if ref is None:
        ref = _REF[blk] = O.parse(blk, ndjson=True, copy_strings=True)
        ref.tape.flags.writeable = False
        ref.strings.flags.writeable = False
    return ref


def assert_block(got, blk, what=""):
    """got = (tape, strings, message) of one delivered result: the oracle's ParseND of `blk`"""
    tape, strings, msg = got
    ref = oracle(blk)
    assert ref.rc == 0, (what, "the oracle rejects this block", ref.rc)
    assert len(tape) == len(ref.tape) and len(strings) == len(ref.strings), (what, len(tape), len(ref.tape), len(strings), len(ref.strings))
    assert np.array_equal(tape, ref.tape), (what, "tape differs at", np.nonzero(np.asarray(tape) != ref.tape)[0][:5])
    assert np.array_equal(strings, ref.strings), (what, "strings differ at", np.nonzero(np.asarray(strings) != ref.strings)[0][:5])
    assert bytes(msg) == blk[ref.msg_off:ref.msg_off + ref.msg_len], (what, "message differs")


def matching_lines(blk, key, value):
    """the lines of `blk` whose root object has `key` with the value `value` (decoded, not searched for as a substring)"""
    out = []
    for ln in blk.split(b"\n"):
        if not ln.strip():
            continue
        doc = json.loads(ln)
        if isinstance(doc, dict) and doc.get(key) == value:
            out.append(ln)
    return out


def assert_filtered(got, records, blk, key, value, what=""):
    """got = (tape, strings) of a filtered result: ParseND of the block's matching lines; the empty result without one"""
    tape, strings = got
    want = matching_lines(blk, key, value)
    assert records == len(want), (what, records, len(want))
    if not want:
        assert len(tape) == 0 and len(strings) == 0, (what, len(tape), len(strings))
        return
    ref = oracle(b"\n".join(want))
    assert ref.rc == 0
    assert len(tape) == len(ref.tape) and len(strings) == len(ref.strings), (what, len(tape), len(ref.tape), len(strings), len(ref.strings))
    assert np.array_equal(tape, ref.tape), (what, "filtered tape differs")
    assert np.array_equal(strings, ref.strings), (what, "filtered strings differ")


# ---- inputs whose blocks are known before the cutter runs -----------------------------------------------------------------
def fill(lines, block_size, first=()):
    """One block of the cutter: the lines of `first`, then lines drawn from the iterator `lines` until the block is longer
    than block_size.  The cutter reads block_size bytes and then the rest of the line, so a segment whose last line starts
    at or before byte block_size and ends after it is cut off as exactly one block, whatever follows it."""
    seg = b"".join(ln + b"\n" for ln in first)
    while len(seg) <= block_size:
        seg += next(lines) + b"\n"
    return seg


def dense_lines(start=0):
    """many tiny records: a large tape and next to nothing in Strings.B (one key in sixteen records)"""
    i = start
    while True:
        yield (b'{"a":%d}' if i % 16 == 5 else b"[%d]") % (i % 10)
        i += 1


def long_string_lines(start=0, n=1800):
    """few records with long strings: a small tape and a large Strings.B"""
    i = start
    while True:
        yield b'{"s":"' + bytes([97 + i % 26]) * (n + i % 7) + b'"}'
        i += 1


def one_record(block_size, extra=100):
    """a single record just over the block size"""
    return b'{"big":"' + b"y" * (block_size + extra - 12) + b'"}\n'


BAD_STAGE1 = b'{"a":"x\x01y"}'   # a raw control byte inside a string
BAD_STAGE2 = b'{"a":1,}'         # a comma in front of the closing brace


# ---- the C API, as it is ------------------------------------------------------------------------------------------------------
class Raw:
    """sjhip_stream_* through ctypes with nothing in between; next and destroy go through bounded()"""

    def __init__(self, block_bytes, slots, n_devices=1):
        import sjhip
        from sjhip import _lib
        self.L = sjhip.lib()
        self._Result = _lib.StreamResult
        self.h = self.L.sjhip_stream_create(0, n_devices, block_bytes, slots, 0)
        assert self.h, "sjhip_stream_create failed"

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.destroy()

    def destroy(self):
        if self.h:
            h, self.h = self.h, None
            bounded(self.L.sjhip_stream_destroy, h)

    def slots(self):
        return self.L.sjhip_stream_slots(self.h)

    def block_capacity(self):
        return self.L.sjhip_stream_block_capacity(self.h)

    def in_flight(self):
        return self.L.sjhip_stream_in_flight(self.h)

    def ready(self):
        return self.L.sjhip_stream_ready(self.h)

    def last_error(self):
        return self.L.sjhip_stream_last_error(self.h).decode()

    def acquire(self):
        ptr, cap = C.c_void_p(), C.c_size_t()
        rc = self.L.sjhip_stream_acquire(self.h, C.byref(ptr), C.byref(cap))
        return rc, ptr.value, cap.value

    def grow(self, keep, new_capacity):
        ptr = C.c_void_p()
        rc = self.L.sjhip_stream_grow(self.h, keep, new_capacity, C.byref(ptr))
        return rc, ptr.value

    def submit(self, n):
        return self.L.sjhip_stream_submit(self.h, n)

    def cancel(self):
        return self.L.sjhip_stream_cancel(self.h)

    def release(self):
        return self.L.sjhip_stream_release(self.h)

    def submit_copy(self, data):
        data = bytes(data)
        return self.L.sjhip_stream_submit_copy(self.h, data, len(data))

    def set_filter(self, key, value):
        return self.L.sjhip_stream_set_filter(self.h, key, len(key), value, len(value))

    def put(self, data):
        """acquire + fill + submit of a block within the capacity -> the slot's block pointer"""
        rc, ptr, cap = self.acquire()
        assert rc == OK and len(data) <= cap, (rc, len(data), cap)
        C.memmove(ptr, bytes(data), len(data))
        assert self.submit(len(data)) == OK
        return ptr

    def next(self):
        """-> (rc, result struct); the pointers of the struct are valid until release()"""
        r = self._Result()
        rc = bounded(self.L.sjhip_stream_next, self.h, C.byref(r))
        return rc, r

    def wait_ready(self):
        """polls ready() until it is 1, with the bound of every other wait"""
        end = time.perf_counter() + JOIN_S
        while not self.ready():
            assert time.perf_counter() < end, f"sjhip_stream_ready still 0 after {JOIN_S} s"
            time.sleep(0.0005)

    def take(self):
        """next + copy + release -> (rc, (tape, strings, message) or None, records)"""
        rc, r = self.next()
        if rc != OK:
            return rc, None, 0
        got = copy_result(r)
        assert self.release() == OK
        return rc, got, int(r.records)


def copy_result(r):
    tape = np.empty(r.tape_len, np.uint64)
    strings = np.empty(r.strings_len, np.uint8)
    if r.tape_len:
        C.memmove(tape.ctypes.data, r.tape, r.tape_len * 8)
    if r.strings_len:
        C.memmove(strings.ctypes.data, r.strings, r.strings_len)
    return tape, strings, C.string_at(r.message, r.message_len) if r.message_len else b""


def run_raw(raw, blocks):
    """Feeds `blocks` with submit_copy, as many in flight as the stream has slots, taking the oldest result whenever the
    stream is full and all of them at the end.  -> (results, rc that ended it: EMPTY after a clean end)"""
    got = []
    for blk in blocks:
        rc = raw.submit_copy(blk)
        if rc == FULL:
            rc, res, _ = raw.take()
            if rc != OK:
                return got, rc
            got.append(res)
            rc = raw.submit_copy(blk)
        assert rc == OK, (rc, raw.last_error())
    while True:
        rc, res, _ = raw.take()
        if rc != OK:
            return got, rc
        got.append(res)


END = object()


def drain(it, keep=lambda pj: (pj.Tape.copy(), pj.Strings.copy(), bytes(pj.Message)), after=None):
    """Every step of the generator `it` under the bound.  -> [keep(pj), ...]; a ParseError of the stream passes through,
    with what was delivered before it in its `delivered` attribute."""
    got = []
    try:
        while True:
            pj = bounded(next, it, END)
            if pj is END:
                return got
            got.append(keep(pj) + (int(pj.records),))
            if after is not None:
                after(pj)
    except Exception as e:
        e.delivered = got
        raise
