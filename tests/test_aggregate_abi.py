"""CPU: libsjhip.so exports sjhip_aggregate_path and sjhip_aggregate_path_records with the argument counts of the header, and
sjhip_agg is 88 bytes in the header and in the ctypes mirror, field for field."""
import ctypes as C
import os
import re

import __graft_entry__ as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sjhip.h")).read(), flags=re.S)


def test_library_exports_the_aggregates():
    L = C.CDLL(G.build_lib())
    import sjhip
    for name, n_args in (("sjhip_aggregate_path", 6), ("sjhip_aggregate_path_records", 13)):
        assert hasattr(L, name) and hasattr(sjhip.lib(), name)
        res, args = sjhip._lib.SYMBOLS[name]
        assert res is C.c_int and len(args) == n_args
        decl = re.search(r"\bint %s\((.*?)\);" % name, HDR, flags=re.S).group(1)
        assert len(decl.split(",")) == n_args, decl
    assert hasattr(sjhip.Context, "aggregate_path") and hasattr(sjhip.Context, "aggregate_path_records")


def test_sjhip_agg_is_88_bytes():
    import aggregate_walk as AW
    import sjhip
    body = re.search(r"typedef struct sjhip_agg \{(.*?)\} sjhip_agg;", HDR, flags=re.S).group(1)
    fields = []  # (name, elements) of the uint64_t members, in order
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        assert decl.startswith("uint64_t "), decl
        for name in decl[len("uint64_t "):].split(","):
            m = re.fullmatch(r"\s*(\w+)(?:\[(\d+)\])?\s*", name)
            fields.append((m.group(1), int(m.group(2) or 1)))
    assert fields == [("rows", 1), ("status", 6), ("sum_lo", 1), ("sum_hi", 1), ("min", 1), ("max", 1)]
    assert 8 * sum(n for _, n in fields) == 88 == C.sizeof(sjhip._lib.Agg)
    assert [(n, C.sizeof(t) // 8) for n, t in sjhip._lib.Agg._fields_] == fields
    assert sjhip.Context.AGG_TILE == AW.AGG_TILE
    assert int(re.search(r"static constexpr int AGG_TILE = (\d+);", open(os.path.join(ROOT, "simdjson-go_amd", "csrc", "query.hip")).read()).group(1)) == AW.AGG_TILE
