"""CPU: libsjhip.so exports sjhip_marshal_rows and sjhip_fetch_marshaled_rows, the header declares them, and the Python mirror binds
them (Context.marshal_rows)."""
import os
import re

import sjhip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_and_header_declares_marshal_rows():
    L = sjhip.lib()
    header = open(os.path.join(ROOT, "include", "sjhip.h")).read()
    for name in ("sjhip_marshal_rows", "sjhip_fetch_marshaled_rows"):
        assert hasattr(L, name), name
        assert re.search(r"^int %s\(sjhip_ctx \*ctx, " % name, header, re.M), name


def test_python_mirror_binds_marshal_rows():
    import ctypes as C
    res, args = sjhip._lib.SYMBOLS["sjhip_marshal_rows"]
    assert res is C.c_int and len(args) == 3
    res, args = sjhip._lib.SYMBOLS["sjhip_fetch_marshaled_rows"]
    assert res is C.c_int and len(args) == 3
    assert callable(getattr(sjhip.Context, "marshal_rows", None))
