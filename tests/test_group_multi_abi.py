"""CPU: libsjhip.so and the Python mirror export sjhip_group_paths, sjhip_fetch_group_keys and sjhip_fetch_group_aggregates_at with
the argument counts of the header; the Go shim (go/simdjson_hip.go) declares the binding and calls the three symbols; the three constants are the same in the header, the mirror and the checker
(tests/group_multi_walk.py); and the extended sizes of a grouping go through the one `groups` product of the result state (publish,
begin, drop: csrc/sj_result.h, replayed by the compiled selftest) with no transition of their own."""
import ctypes as C
import json
import os
import re

import __graft_entry__ as G
import group_multi_walk as MW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sjhip.h")).read(), flags=re.S)
CALLS = (("sjhip_group_paths", 13), ("sjhip_fetch_group_keys", 6), ("sjhip_fetch_group_aggregates_at", 8))


def test_library_exports_the_calls():
    L = C.CDLL(G.build_lib())
    import sjhip
    for name, n_args in CALLS:
        assert hasattr(L, name) and hasattr(sjhip.lib(), name), name
        res, args = sjhip._lib.SYMBOLS[name]
        assert res is C.c_int and len(args) == n_args, name
        decl = re.search(r"\bint %s\((.*?)\);" % name, HDR, flags=re.S).group(1)
        assert len(decl.split(",")) == n_args, decl
    for method in ("group_paths", "fetch_group_paths", "fetch_group_keys", "fetch_group_aggregates_at", "group_path", "fetch_groups"):
        assert hasattr(sjhip.Context, method), method


def test_go_binding_declares_and_calls_them():
    """the Go identifier list of the shim (tools/check_go_collisions.py scan_go) holds the binding, and its cgo calls name the three
    symbols and the three constants (their argument counts against the header: tests/test_go_binding.py)"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_go_collisions as GO
    with open(GO.SHIM) as f:
        shim = f.read()
    decls = GO.scan_go(shim)["decls"]
    for name in ("ViewParser.GroupPaths", "GroupKeyColumn", "GroupValueColumn", "GroupKeys", "GroupAggregates", "GroupsResult", "GroupNone",
                 "GroupMaxKeys", "GroupMaxValues", "GroupString", "GroupInt", "GroupUint", "GroupBool", "GroupFloat"):
        assert name in decls, (name, decls)
    used = set(re.findall(r"\bC\.(sjhip_[a-z0-9_]+|SJHIP_[A-Z0-9_]+)", GO.strip_go(shim)))
    assert {name for name, _ in CALLS} | {"sjhip_fetch_groups", "SJHIP_GROUP_MAX_KEYS", "SJHIP_GROUP_MAX_VALUES", "SJHIP_GROUP_NULL_KEY",
                                          "SJHIP_GROUP_NONE"} <= used, used
    assert GO.check(shim, json.load(open(GO.INVENTORY))["files"]) == []  # no identifier of the reference's package is declared again
    kinds = dict(re.findall(r"\b(Group(?:Float|Int|Uint|Bool|String))\s+GroupColumnKind = (\d)", shim))
    enum = dict(re.findall(r"SJHIP_COL_(FLOAT|INT|UINT|BOOL|STRING) = (\d)", HDR))
    assert {k[5:].upper(): v for k, v in kinds.items()} == enum and len(enum) == 5


def test_the_three_constants():
    import sjhip
    keys = int(re.search(r"#define SJHIP_GROUP_MAX_KEYS (\d+)\b", HDR).group(1))
    values = int(re.search(r"#define SJHIP_GROUP_MAX_VALUES (\d+)\b", HDR).group(1))
    null_key = int(re.search(r"#define SJHIP_GROUP_NULL_KEY (\d+)u\b", HDR).group(1))
    assert keys == 8 == sjhip.Context.GROUP_MAX_KEYS == MW.GROUP_MAX_KEYS
    assert values == 8 == sjhip.Context.GROUP_MAX_VALUES == MW.GROUP_MAX_VALUES
    assert null_key == 1 == sjhip.Context.GROUP_NULL_KEY == MW.GROUP_NULL_KEY


def test_extended_sizes_go_through_the_groups_product():
    lib = C.CDLL(G.build_selftest())
    out = (C.c_uint64 * 11)()
    assert lib.sj_selftest_groups_sizes(out) == MW.GROUP_MAX_KEYS == MW.GROUP_MAX_VALUES
    # published on a parsed state, given up by its own begin, published again, dropped by a parse, not published without a result
    assert list(out[:5]) == [1, 0, 1, 0, 0]
    assert list(out[5:]) == [2, 2, 1, 2, 24, 3]
