"""CPU: libsjhip.so and the Python mirror export sjhip_order_paths with the argument count of the header; SJHIP_ORDER_MAX_KEYS is the
same in the header, in csrc/sj_order.h and in the mirror; and the two host-and-device helpers of the device's plan (csrc/sj_order.h
mkord_class_key and mkord_stays, replayed by the compiled selftest) are the checker's (tests/order_multi_walk.py class_key, stays)."""
import ctypes as C
import os
import re

import __graft_entry__ as G
import order_multi_walk as MW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sjhip.h")).read(), flags=re.S)


def test_library_exports_the_call():
    L = C.CDLL(G.build_lib())
    import sjhip
    name, n_args = "sjhip_order_paths", 10
    assert hasattr(L, name) and hasattr(sjhip.lib(), name)
    res, args = sjhip._lib.SYMBOLS[name]
    assert res is C.c_int and len(args) == n_args
    decl = re.search(r"\bint %s\((.*?)\);" % name, HDR, flags=re.S).group(1)
    assert len(decl.split(",")) == n_args, decl
    assert hasattr(sjhip.Context, "order_paths") and sjhip.Context.ORDER_DESC == MW.ORDER_DESC


def test_the_column_limit_is_one_number():
    import sjhip
    lib = C.CDLL(G.build_selftest())
    in_header = int(re.search(r"#define SJHIP_ORDER_MAX_KEYS (\d+)\b", HDR).group(1))
    assert in_header == 8 == lib.sj_selftest_order_max_keys() == sjhip.Context.ORDER_MAX_KEYS == MW.ORDER_MAX_KEYS


def test_class_key_and_stays_are_the_checkers():
    lib = C.CDLL(G.build_selftest())
    lib.sj_selftest_mkord_class_key.argtypes = [C.c_uint32, C.c_int]
    lib.sj_selftest_mkord_class_key.restype = C.c_uint32
    for cls in (0, 1, 2, 127, 128, 255, 256, 65535, 65536, (1 << 30) - 1, 1 << 30):
        for missing in (0, 1):
            assert lib.sj_selftest_mkord_class_key(cls, missing) == MW.class_key(cls, bool(missing)), (cls, missing)
    # the missing rows of a class lie behind its others and in front of the next class
    keys = [MW.class_key(c, m) for c in (1, 2, 3) for m in (False, True)]
    assert keys == sorted(keys) and len(set(keys)) == 6
    for missing in (0, 1):
        for alone in (0, 1):
            for full in (0, 1):
                assert bool(lib.sj_selftest_mkord_stays(missing, alone, full)) == MW.stays(bool(missing), bool(alone), bool(full))
