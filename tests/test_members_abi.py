"""CPU: libsjhip.so exports sjhip_unnest_members, sjhip_extract_row_names and sjhip_where_row_names with the argument counts of the
header, and the Python mirror declares and wraps them."""
import ctypes as C
import os
import re

import __graft_entry__ as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sjhip.h")).read(), flags=re.S)


def test_library_exports_the_member_calls():
    L = C.CDLL(G.build_lib())
    import sjhip
    for name, n_args in (("sjhip_unnest_members", 7), ("sjhip_extract_row_names", 3), ("sjhip_where_row_names", 7)):
        assert hasattr(L, name) and hasattr(sjhip.lib(), name)
        res, args = sjhip._lib.SYMBOLS[name]
        assert res is C.c_int and len(args) == n_args
        decl = re.search(r"\bint %s\((.*?)\);" % name, HDR, flags=re.S).group(1)
        assert len(decl.split(",")) == n_args, decl
    for method in ("unnest_members", "extract_row_names", "where_row_names"):
        assert hasattr(sjhip.Context, method)
