"""CPU: libsjhip.so exports sjhip_order_path and sjhip_fetch_order with the argument counts of the header, SJHIP_ORDER_DESC is in the
header and in the Python mirror, and the tile constants of the checker (tests/order_walk.py) are the ones of the source."""
import ctypes as C
import os
import re

import __graft_entry__ as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "simdjson-go_amd", "csrc")
HDR = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sjhip.h")).read(), flags=re.S)


def test_library_exports_the_order_calls():
    L = C.CDLL(G.build_lib())
    import sjhip
    for name, n_args in (("sjhip_order_path", 9), ("sjhip_fetch_order", 4)):
        assert hasattr(L, name) and hasattr(sjhip.lib(), name)
        res, args = sjhip._lib.SYMBOLS[name]
        assert res is C.c_int and len(args) == n_args
        decl = re.search(r"\bint %s\((.*?)\);" % name, HDR, flags=re.S).group(1)
        assert len(decl.split(",")) == n_args, decl
    assert hasattr(sjhip.Context, "order_path") and hasattr(sjhip.Context, "fetch_order") and hasattr(sjhip, "Order")


def test_constants():
    import order_walk as OW
    import sjhip
    assert re.search(r"#define SJHIP_ORDER_DESC 1u\b", HDR)
    assert sjhip.Context.ORDER_DESC == OW.ORDER_DESC == 1
    import group_walk as GW
    src = open(os.path.join(CSRC, "sj_sort.h")).read()  # (the one sort of the grouping and the ordering)

    def const(name, text=src):
        return int(re.search(r"\b%s = (\d+)\b" % name, text).group(1))
    assert const("SORT_RADIX_BITS") == OW.ORDER_RADIX_BITS == GW.GROUP_RADIX_BITS
    assert (const("SORT_THREADS"), const("SORT_ROUNDS")) == (OW.ORDER_SORT_THREADS, OW.ORDER_SORT_ROUNDS)
    assert (const("SORT_THREADS"), const("SORT_ROUNDS")) == (GW.GROUP_SORT_THREADS, GW.GROUP_SORT_ROUNDS)
    assert re.search(r"\bSORT_TILE = SORT_THREADS \* SORT_ROUNDS;", src)
    assert sjhip.Context.ORDER_SORT_TILE == OW.ORDER_SORT_TILE == OW.ORDER_SORT_THREADS * OW.ORDER_SORT_ROUNDS
    assert sjhip.Context.GROUP_SORT_TILE == GW.GROUP_SORT_TILE == OW.ORDER_SORT_TILE
    walk = open(os.path.join(CSRC, "sj_tapewalk.h")).read()
    assert re.search(r"QT = TW_THREADS, QI = 4, QTILE = QT \* QI;", walk) and const("TW_THREADS", walk) * 4 == OW.QTILE
    # ... and of the compiled selftest (what the kernels are built with)
    lib = C.CDLL(G.build_selftest())
    out = (C.c_int * 4)()
    lib.sj_selftest_order_geometry(out)
    assert list(out) == [OW.ORDER_RADIX_BITS, OW.ORDER_SORT_THREADS, OW.ORDER_SORT_ROUNDS, OW.ORDER_SORT_TILE]
