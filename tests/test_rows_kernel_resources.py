"""The kernels of the row selection (sjhip_select_rows, query.hip) exist, stay off scratch -- the tile pass keeps its eight words
and its masks in registers, no per-lane array -- and leave room for at least 4 waves per SIMD; the table kernel, which now starts
at a row's value, keeps the figures tests/test_table_kernel_resources.py demands.  Compile-only: hipcc's resource remarks
(tools/kernel_resources.py), on the product and on the bounds-checked build."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as KR  # noqa: E402

ROW_KERNELS = ["k_q_rows_records", "k_q_rows_last", "k_q_rows_scan_last", "k_q_rows_offsets"]


@pytest.mark.parametrize("flags", [(), ("-DSJ_DEBUG_BOUNDS",)], ids=["product", "bounds-checked"])
def test_row_kernels_use_no_scratch(flags):
    rows = {}
    for name, vgprs, scratch, occ, lds in KR.kernels_of("query.hip", flags):
        rows.setdefault(name.split("(")[0].split("<")[0].split(" ")[-1], []).append((name, vgprs, scratch, occ, lds))
    for kernel in ROW_KERNELS:
        assert len(rows.get(kernel, [])) == 1, (kernel, sorted(rows))
    assert len(rows.get("k_q_rows_tile", [])) == 3, sorted(rows)  # the depth sums, the count, the compaction
    for kernel in ROW_KERNELS + ["k_q_rows_tile"]:
        for name, vgprs, scratch, occ, lds in rows[kernel]:
            assert scratch == 0, (name, vgprs, scratch, occ, lds)
            assert occ >= 4, (name, vgprs, scratch, occ, lds)
    (name, vgprs, scratch, occ, lds), = rows["k_q_table_walk"]
    assert scratch == 0 and occ >= 4 and lds == 2 * 16 * 4 * 256, rows["k_q_table_walk"]
