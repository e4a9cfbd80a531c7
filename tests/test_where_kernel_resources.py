"""The kernels of the row predicates (sjhip_where_path, query.hip) exist exactly once, stay off scratch and leave room for at least
4 waves per SIMD; the table kernel and the kernels of the row selection keep the figures tests/test_table_kernel_resources.py and
tests/test_rows_kernel_resources.py demand of them.  Compile-only: hipcc's resource remarks (tools/kernel_resources.py), on the
product and on the bounds-checked build."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as KR  # noqa: E402

from test_rows_kernel_resources import ROW_KERNELS  # noqa: E402

WHERE_KERNELS = ["k_q_where_mark", "k_q_where_apply", "k_q_where_offsets"]


@pytest.mark.parametrize("flags", [(), ("-DSJ_DEBUG_BOUNDS",)], ids=["product", "bounds-checked"])
def test_where_kernels_use_no_scratch(flags):
    rows = {}
    for name, vgprs, scratch, occ, lds in KR.kernels_of("query.hip", flags):
        rows.setdefault(name.split("(")[0].split("<")[0].split(" ")[-1], []).append((name, vgprs, scratch, occ, lds))
    for kernel in WHERE_KERNELS + ROW_KERNELS + ["k_q_count_path"]:
        assert len(rows.get(kernel, [])) == 1, (kernel, sorted(rows))
    assert len(rows.get("k_q_rows_tile", [])) == 3, sorted(rows)
    for kernel in WHERE_KERNELS + ROW_KERNELS + ["k_q_rows_tile", "k_q_count_path"]:
        for name, vgprs, scratch, occ, lds in rows[kernel]:
            assert scratch == 0, (name, vgprs, scratch, occ, lds)
            assert occ >= 4, (name, vgprs, scratch, occ, lds)
    (name, vgprs, scratch, occ, lds), = rows["k_q_table_walk"]
    assert scratch == 0 and occ >= 4 and lds == 2 * 16 * 4 * 256, rows["k_q_table_walk"]
