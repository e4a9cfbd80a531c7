"""The kernel of the tables (sjhip_extract_table, query.hip) exists, stays off scratch -- its walk keeps the matched nodes in a
mask and its resume stack in LDS, no per-lane array -- and leaves room for at least 4 waves per SIMD beside its 32 KiB of LDS
per block.  Compile-only: hipcc's resource remarks (tools/kernel_resources.py), on the product and on the bounds-checked build."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as KR  # noqa: E402


@pytest.mark.parametrize("flags", [(), ("-DSJ_DEBUG_BOUNDS",)], ids=["product", "bounds-checked"])
def test_table_walk_uses_no_scratch(flags):
    rows = {name.split("(")[0]: (vgprs, scratch, occ, lds) for name, vgprs, scratch, occ, lds in KR.kernels_of("query.hip", flags)}
    assert "k_q_table_walk" in rows, sorted(rows)
    vgprs, scratch, occ, lds = rows["k_q_table_walk"]
    assert scratch == 0, rows["k_q_table_walk"]
    assert occ >= 4, rows["k_q_table_walk"]  # (the one-lane-per-record walk hides its latency behind other waves)
    assert lds == 2 * 16 * 4 * 256, rows["k_q_table_walk"]  # the resume stack: two u32 for each of 16 levels and 256 lanes
