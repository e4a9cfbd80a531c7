"""CPU: libsjhip.so and the Python mirror export sjhip_order_path_strings with the argument count of the header, and the chunk key of
the device's rounds (csrc/sj_order.h strord_chunk, replayed by the compiled selftest) is the checker's (tests/order_strings_walk.py
chunk) for key lengths 0 .. 15 at the offsets 0, 7 and 14, in both directions."""
import ctypes as C
import os
import re

import __graft_entry__ as G
import order_strings_walk as SW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "simdjson-go_amd", "csrc")
HDR = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sjhip.h")).read(), flags=re.S)


def test_library_exports_the_call():
    L = C.CDLL(G.build_lib())
    import sjhip
    name, n_args = "sjhip_order_path_strings", 8
    assert hasattr(L, name) and hasattr(sjhip.lib(), name)
    res, args = sjhip._lib.SYMBOLS[name]
    assert res is C.c_int and len(args) == n_args
    decl = re.search(r"\bint %s\((.*?)\);" % name, HDR, flags=re.S).group(1)
    assert len(decl.split(",")) == n_args, decl
    assert hasattr(sjhip.Context, "order_path_strings") and sjhip.Context.COL_STRING == SW.COL_STRING
    assert sjhip.Context.ORDER_DESC == SW.ORDER_DESC


def test_chunk_key_is_the_checkers():
    lib = C.CDLL(G.build_selftest())
    lib.sj_selftest_strord_chunk.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_int, C.POINTER(C.c_uint64)]
    lib.sj_selftest_strord_chunk.restype = None
    src = open(os.path.join(CSRC, "sj_order.h")).read()
    assert int(re.search(r"\bSTRORD_CHUNK = (\d+)\b", src).group(1)) == SW.CHUNK
    pattern = [0x00, 0x7F, 0x80, 0xFF, 0x61, 0x00, 0xFF, 0x80, 0x7F, 0x00, 0x01, 0xFE, 0x00, 0x00, 0xFF]
    seen = set()
    for first in range(4):  # every one of 0x00, 0x7F, 0x80, 0xFF leads a chunk at every offset
        rotated = pattern[first:] + pattern[:first]
        for length in range(16):
            key = bytes(rotated[:length])
            for at in (0, 7, 14):
                for desc in (0, 1):
                    out = (C.c_uint64 * 3)()
                    lib.sj_selftest_strord_chunk(key, length, at, desc, out)
                    want = SW.chunk(key, at, bool(desc))
                    assert out[0] == want, (key, at, desc, hex(out[0]), hex(want))
                    assert out[1] == max(0, min(SW.CHUNK, length - at)) and out[2] == SW.max_rounds(length)
                    seen.add(out[0])
    assert len(seen) > 100
    # the order of the chunk keys is bytes.Compare on the chunks
    keys = [b"", b"a", b"a\0", b"a\0\0", b"a\0b", b"a\1", b"b", b"\x7f", b"\x80", b"\xff" * 7]
    assert sorted(keys, key=lambda k: SW.chunk(k, 0)) == sorted(keys) and sorted(keys, key=lambda k: SW.chunk(k, 0, True)) == sorted(keys, reverse=True)
