"""CPU: include/sjhip.h declares sjhip_row_schema and sjhip_fetch_row_schema, the SJHIP_TYPE_* values and SJHIP_SCHEMA_TYPES;
libsjhip.so exports both functions with the argument counts of the header; the Python mirror declares and wraps them and exports
the TYPE_* constants; and a C11 caller compiles against the header and links the two symbols."""
import ctypes as C
import os
import re
import subprocess

import __graft_entry__ as G

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "simdjson-go_amd")
RAW = open(os.path.join(ROOT, "include", "sjhip.h")).read()
HDR = re.sub(r"/\*.*?\*/", "", RAW, flags=re.S)
TYPES = {"NULL": 1, "STRING": 2, "INT": 3, "UINT": 4, "FLOAT": 5, "BOOL": 6, "OBJECT": 7, "ARRAY": 8}  # the reference's Type values

CALLER = r"""
#include <stdio.h>
#include "sjhip.h"
_Static_assert(SJHIP_TYPE_NULL == 1 && SJHIP_TYPE_STRING == 2 && SJHIP_TYPE_INT == 3 && SJHIP_TYPE_UINT == 4, "Type values");
_Static_assert(SJHIP_TYPE_FLOAT == 5 && SJHIP_TYPE_BOOL == 6 && SJHIP_TYPE_OBJECT == 7 && SJHIP_TYPE_ARRAY == 8, "Type values");
_Static_assert(SJHIP_SCHEMA_TYPES == SJHIP_TYPE_ARRAY, "one column per type");
int main(void) {
    int (*schema)(sjhip_ctx *, const uint8_t *, const uint32_t *, uint32_t, size_t *, uint64_t[6], uint64_t *, size_t *, size_t *) = sjhip_row_schema;
    int (*fetch)(sjhip_ctx *, uint64_t *, uint8_t *, uint64_t *, uint64_t *) = sjhip_fetch_row_schema;
    size_t rows = 0, names = 0, bytes = 0;
    uint64_t status[6], members = 0, counts[SJHIP_SCHEMA_TYPES];
    /* without a context both calls refuse and touch nothing */
    int bad = schema(NULL, NULL, NULL, 0, &rows, status, &members, &names, &bytes) != SJHIP_ERR_ARG;
    bad += fetch(NULL, NULL, NULL, NULL, counts) != SJHIP_ERR_ARG;
    printf("%d\n", bad);
    return bad;
}
"""


def test_header_declares_the_schema_calls():
    for name, value in TYPES.items():
        assert re.search(r"\bSJHIP_TYPE_%s = %d\b" % (name, value), HDR), name
    assert re.search(r"#define SJHIP_SCHEMA_TYPES 8\b", HDR)
    for name, n_args in (("sjhip_row_schema", 9), ("sjhip_fetch_row_schema", 5)):
        decl = re.search(r"\bint %s\((.*?)\);" % name, HDR, flags=re.S).group(1)
        assert len(decl.split(",")) == n_args, decl
    assert "uint64_t status[6]" in HDR and "sjhip_row_schema" in RAW.split("sjhip_fetch_row_schema")[0]


def test_library_exports_the_schema_calls():
    L = C.CDLL(G.build_lib())
    import sjhip
    for name, n_args in (("sjhip_row_schema", 9), ("sjhip_fetch_row_schema", 5)):
        assert hasattr(L, name) and hasattr(sjhip.lib(), name)
        res, args = sjhip._lib.SYMBOLS[name]
        assert res is C.c_int and len(args) == n_args
    for method in ("row_schema", "fetch_row_schema"):
        assert hasattr(sjhip.Context, method)
    for name, value in TYPES.items():
        assert getattr(sjhip, "TYPE_" + name) == getattr(sjhip.Context, "TYPE_" + name) == value
    assert sjhip.Context.SCHEMA_TYPES == 8 and sjhip.Schema


def test_c11_caller_compiles_and_links(tmp_path):
    G.build_lib()
    src, exe = tmp_path / "schema_caller.c", tmp_path / "schema_caller"
    src.write_text(CALLER)
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", PKG, "-lsjhip", f"-Wl,-rpath,{PKG}"])
    out = subprocess.run([str(exe)], capture_output=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == b"0", (out.returncode, out.stdout, out.stderr)
