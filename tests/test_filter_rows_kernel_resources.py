"""The kernels of sjhip_filter_rows (query.hip) exist exactly once, stay off scratch and leave room for at least 4 waves per SIMD;
the kernels of the row predicates and of the row selection keep the figures tests/test_where_kernel_resources.py demands of them.
Compile-only: hipcc's resource remarks (tools/kernel_resources.py), on the product and on the bounds-checked build."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as KR  # noqa: E402

from test_rows_kernel_resources import ROW_KERNELS  # noqa: E402
from test_where_kernel_resources import WHERE_KERNELS  # noqa: E402

FILTER_ROWS_KERNELS = ["k_q_frows_measure", "k_q_frows_tile_sums", "k_q_frows_tile_apply", "k_q_frows_copy"]


@pytest.mark.parametrize("flags", [(), ("-DSJ_DEBUG_BOUNDS",)], ids=["product", "bounds-checked"])
def test_filter_rows_kernels_use_no_scratch(flags):
    rows = {}
    for name, vgprs, scratch, occ, lds in KR.kernels_of("query.hip", flags):
        rows.setdefault(name.split("(")[0].split("<")[0].split(" ")[-1], []).append((name, vgprs, scratch, occ, lds))
    for kernel in FILTER_ROWS_KERNELS + WHERE_KERNELS + ROW_KERNELS + ["k_q_copy", "k_q_mark"]:
        assert len(rows.get(kernel, [])) == 1, (kernel, sorted(rows))
    assert len(rows.get("k_q_rows_tile", [])) == 3, sorted(rows)
    for kernel in FILTER_ROWS_KERNELS + WHERE_KERNELS + ROW_KERNELS + ["k_q_rows_tile"]:
        for name, vgprs, scratch, occ, lds in rows[kernel]:
            assert scratch == 0, (name, vgprs, scratch, occ, lds)
            assert occ >= 4, (name, vgprs, scratch, occ, lds)
