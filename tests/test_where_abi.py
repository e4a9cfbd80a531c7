"""CPU: libsjhip.so exports sjhip_where_path, the header numbers the new operators as the ABI states them, and the Python mirror
declares the call and the operators."""
import ctypes as C
import os
import re

import __graft_entry__ as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_where_path():
    L = C.CDLL(G.build_lib())
    assert hasattr(L, "sjhip_where_path")
    import sjhip
    res, args = sjhip._lib.SYMBOLS["sjhip_where_path"]
    assert res is C.c_int and len(args) == 10
    assert hasattr(sjhip.lib(), "sjhip_where_path")


def test_operator_numbers():
    import sjhip
    import where_walk as WW
    hdr = open(os.path.join(ROOT, "include", "sjhip.h")).read()
    body = re.search(r"enum \{ SJHIP_OP_EXISTS = 0,(.*?)\};", hdr, flags=re.S).group(1)
    names = ["SJHIP_OP_EXISTS"] + re.findall(r"\b(SJHIP_OP_[A-Z_]+)", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert len(names) == 20 and names[7] == "SJHIP_OP_LT_INT" and names[19] == "SJHIP_OP_PREFIX_STRING"
    assert "SJHIP_OP_LT_INT = 7" in body and re.search(r"#define SJHIP_WHERE_NOT 1u", hdr)
    for number, name in enumerate(names):
        short = name[len("SJHIP_"):]
        assert getattr(sjhip.Context, short) == number, name
        if number >= 7:
            assert getattr(WW, short) == number, name
    assert sjhip.Context.WHERE_NOT == 1
