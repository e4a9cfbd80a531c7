"""CPU: libsjhip.so exports sjhip_marshal_rows_paths, the header declares it with SJHIP_PROJECT_NULLS, and the Python mirror binds
it with its 10 arguments (Context.marshal_rows_paths)."""
import os
import re

import sjhip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_and_header_declares_marshal_rows_paths():
    L = sjhip.lib()
    header = open(os.path.join(ROOT, "include", "sjhip.h")).read()
    assert hasattr(L, "sjhip_marshal_rows_paths")
    assert re.search(r"^int sjhip_marshal_rows_paths\(sjhip_ctx \*ctx, const uint8_t \*keys, const uint32_t \*key_lens, const uint32_t \*path_lens,",
                     header, re.M)
    assert re.search(r"^#define SJHIP_PROJECT_NULLS 1u\b", header, re.M)


def test_python_mirror_binds_marshal_rows_paths():
    import ctypes as C
    res, args = sjhip._lib.SYMBOLS["sjhip_marshal_rows_paths"]
    assert res is C.c_int and len(args) == 10
    assert callable(getattr(sjhip.Context, "marshal_rows_paths", None))
    assert sjhip.Context.PROJECT_NULLS == 1
