"""CPU: libsjhip.so exports sjhip_filter_rows, the Python mirror declares its five arguments, and Context has filter_rows."""
import ctypes as C

import __graft_entry__ as G


def test_library_exports_filter_rows():
    L = C.CDLL(G.build_lib())
    assert hasattr(L, "sjhip_filter_rows")
    import sjhip
    res, args = sjhip._lib.SYMBOLS["sjhip_filter_rows"]
    assert res is C.c_int and len(args) == 5
    assert hasattr(sjhip.lib(), "sjhip_filter_rows")
    assert callable(getattr(sjhip.Context, "filter_rows", None))
