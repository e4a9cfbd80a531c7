"""The kernels of the aggregates (sjhip_aggregate_path / sjhip_aggregate_path_records, query.hip) exist exactly once, stay off
scratch and leave room for at least 4 waves per SIMD; the column kernel next to them, the kernels of the row predicates and of the
row selection and the table kernel keep the figures tests/test_where_kernel_resources.py demands of them.  Compile-only: hipcc's
resource remarks (tools/kernel_resources.py), on the product and on the bounds-checked build."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as KR  # noqa: E402

from test_rows_kernel_resources import ROW_KERNELS  # noqa: E402
from test_where_kernel_resources import WHERE_KERNELS  # noqa: E402

AGG_KERNELS = ["k_q_agg_heads", "k_q_agg_rows", "k_q_agg_fold"]


@pytest.mark.parametrize("flags", [(), ("-DSJ_DEBUG_BOUNDS",)], ids=["product", "bounds-checked"])
def test_aggregate_kernels_use_no_scratch(flags):
    rows = {}
    for name, vgprs, scratch, occ, lds in KR.kernels_of("query.hip", flags):
        rows.setdefault(name.split("(")[0].split("<")[0].split(" ")[-1], []).append((name, vgprs, scratch, occ, lds))
    neighbours = WHERE_KERNELS + ROW_KERNELS + ["k_q_count_path", "k_q_extract", "k_q_find_path"]
    for kernel in AGG_KERNELS + neighbours:
        assert len(rows.get(kernel, [])) == 1, (kernel, sorted(rows))
    assert len(rows.get("k_q_rows_tile", [])) == 3, sorted(rows)
    for kernel in AGG_KERNELS + neighbours + ["k_q_rows_tile"]:
        for name, vgprs, scratch, occ, lds in rows[kernel]:
            assert scratch == 0, (name, vgprs, scratch, occ, lds)
            assert occ >= 4, (name, vgprs, scratch, occ, lds)
    (name, vgprs, scratch, occ, lds), = rows["k_q_table_walk"]
    assert scratch == 0 and occ >= 4 and lds == 2 * 16 * 4 * 256, rows["k_q_table_walk"]
