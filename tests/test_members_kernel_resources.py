"""The kernels of the member rows (sjhip_unnest_members, sjhip_extract_row_names, sjhip_where_row_names; query.hip) exist -- one
lane pass over the parents, the count and the write instantiation of the tile pass, the lengths of the names, the mark of the name
predicate --, stay off scratch and leave room for at least 4 waves per SIMD: the bar the kernels of the unnest hold, whose tile
walk they share.  Compile-only: hipcc's resource remarks (tools/kernel_resources.py), on the product and on the bounds-checked
build."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as KR  # noqa: E402

MEMBER_KERNELS = ["k_q_members_parents", "k_q_names_len", "k_q_names_mark"]


@pytest.mark.parametrize("flags", [(), ("-DSJ_DEBUG_BOUNDS",)], ids=["product", "bounds-checked"])
def test_member_kernels_use_no_scratch(flags):
    rows = {}
    for name, vgprs, scratch, occ, lds in KR.kernels_of("query.hip", flags):
        rows.setdefault(name.split("(")[0].split("<")[0].split(" ")[-1], []).append((name, vgprs, scratch, occ, lds))
    for kernel in MEMBER_KERNELS:
        assert len(rows.get(kernel, [])) == 1, (kernel, sorted(rows))
    assert len(rows.get("k_q_members_tile", [])) == 2, sorted(rows)  # the count, the write
    assert sorted(k for k in rows if k.startswith("k_q_members_") or k.startswith("k_q_names_")) == sorted(MEMBER_KERNELS + ["k_q_members_tile"])
    for kernel in MEMBER_KERNELS + ["k_q_members_tile"]:
        for name, vgprs, scratch, occ, lds in rows[kernel]:
            print(name, "vgprs", vgprs, "scratch", scratch, "waves/SIMD", occ, "lds", lds)
            assert scratch == 0, (name, vgprs, scratch, occ, lds)
            assert occ >= 4, (name, vgprs, scratch, occ, lds)
