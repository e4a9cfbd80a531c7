"""CPU: include/sjhip.h declares sjhip_where_path_in, sjhip_count_where_path_in and SJHIP_WHERE_IN_MAX_VALUES; libsjhip.so exports
both functions; the Python mirror and the Go shim (go/simdjson_hip.go) bind them with the argument counts of the header; the
constant is one number in the header, the mirror and the checker (tests/where_in_walk.py); a C11 caller compiles against the header
and links both symbols; and the compiled replay of the set's table (csrc/sj_wherein.h, host_selftest.cpp) agrees with std::set."""
import ctypes as C
import os
import re
import subprocess
import sys

import __graft_entry__ as G
import where_in_walk as IW

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "simdjson-go_amd")
HDR = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sjhip.h")).read(), flags=re.S)
# ctx, keys, key_lens, n_keys, kind, value_offsets, values, n_values, flags = 9, then records and rows / count
N_ARGS = {"sjhip_where_path_in": 11, "sjhip_count_where_path_in": 10}

CALLER = r"""
#include <stdio.h>
#include "sjhip.h"
_Static_assert(SJHIP_WHERE_IN_MAX_VALUES == 16777216u, "the most values of a set");
int main(void) {
    int (*in)(sjhip_ctx *, const uint8_t *, const uint32_t *, uint32_t, int, const uint64_t *, const void *, size_t, uint32_t, size_t *,
              size_t *) = sjhip_where_path_in;
    int (*count)(sjhip_ctx *, const uint8_t *, const uint32_t *, uint32_t, int, const uint64_t *, const void *, size_t, uint32_t,
                 uint64_t *) = sjhip_count_where_path_in;
    size_t records = 7, rows = 7;
    uint64_t n = 7;
    const int64_t values[2] = {1, 2};
    /* without a context both calls refuse and touch nothing */
    int bad = in(NULL, NULL, NULL, 0, SJHIP_COL_INT, NULL, values, 2, SJHIP_WHERE_NOT, &records, &rows) != SJHIP_ERR_ARG;
    bad += count(NULL, NULL, NULL, 0, SJHIP_COL_STRING, NULL, NULL, 0, 0, &n) != SJHIP_ERR_ARG;
    bad += records != 7 || rows != 7 || n != 7;
    printf("%d\n", bad);
    return bad;
}
"""


def test_header_declares_the_calls_and_the_constant():
    assert re.search(r"#define SJHIP_WHERE_IN_MAX_VALUES \(1u << 24\)", HDR)
    for name, n_args in N_ARGS.items():
        decl = re.search(r"\bint %s\((.*?)\);" % name, HDR, flags=re.S).group(1)
        assert len(decl.split(",")) == n_args, decl
        assert "const uint64_t *value_offsets, const void *values, size_t n_values, uint32_t flags" in " ".join(decl.split())


def test_library_and_mirror_bind_the_calls():
    L = C.CDLL(G.build_lib())
    import sjhip
    for name, n_args in N_ARGS.items():
        assert hasattr(L, name) and hasattr(sjhip.lib(), name)
        res, args = sjhip._lib.SYMBOLS[name]
        assert res is C.c_int and len(args) == n_args
    assert hasattr(sjhip.Context, "where_path_in") and hasattr(sjhip.Context, "count_where_path_in")
    assert sjhip.Context.WHERE_IN_MAX_VALUES == IW.WHERE_IN_MAX_VALUES == 1 << 24
    assert sjhip.Context.COL_STRING == IW.COL_STRING and IW.MAX_STRING == 1024


def test_go_binding_declares_and_calls_them():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_go_collisions as GO
    import json
    from test_go_binding import _top_level_args
    with open(GO.SHIM) as f:
        shim = f.read()
    decls = GO.scan_go(shim)["decls"]
    for name in ("ViewParser.WherePathIn", "ViewParser.CountWherePathIn", "WhereInSet", "WhereInMaxValues"):
        assert name in decls, (name, decls)
    stripped = GO.strip_go(shim)
    used = set(re.findall(r"\bC\.(sjhip_[a-z0-9_]+|SJHIP_[A-Z0-9_]+)", stripped))
    assert set(N_ARGS) | {"SJHIP_WHERE_IN_MAX_VALUES", "SJHIP_WHERE_NOT"} <= used, used
    for name, n_args in N_ARGS.items():
        calls = [m.end() - 1 for m in re.finditer(r"\bC\.%s\s*\(" % name, stripped)]
        assert calls and all(_top_level_args(stripped, at) == n_args for at in calls), name
    assert GO.check(shim, json.load(open(GO.INVENTORY))["files"]) == []  # no identifier of the reference's package is declared again


def test_c11_caller_compiles_and_links(tmp_path):
    G.build_lib()
    src, exe = tmp_path / "where_in_caller.c", tmp_path / "where_in_caller"
    src.write_text(CALLER)
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", PKG, "-lsjhip", f"-Wl,-rpath,{PKG}"])
    out = subprocess.run([str(exe)], capture_output=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == b"0", (out.returncode, out.stdout, out.stderr)


def test_compiled_replay_of_the_table_agrees_with_std_set():
    lib = C.CDLL(G.build_selftest())
    out = (C.c_uint64 * 8)()
    assert lib.sj_selftest_where_in(out) == 0, list(out)
    sets, probes, hits, wrapped, equal_hashes, longest = list(out[:6])
    # sets with duplicates, with equal hashes and with chains that wrap were replayed, in several insertion orders
    assert sets >= 12 and probes > 1000 and 0 < hits < probes and wrapped > 0 and equal_hashes > 0 and longest >= 33
