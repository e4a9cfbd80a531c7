"""The kernels of the grouping (sjhip_group_path, query.hip) exist exactly once, stay off scratch and leave room for at least 4 waves
per SIMD -- the bar tests/test_aggregate_kernel_resources.py sets for the aggregates -- and the aggregate kernels, which took the row
permutation of the grouping, and the neighbours named there keep that bar.  Compile-only: hipcc's resource remarks
(tools/kernel_resources.py), on the product and on the bounds-checked build."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as KR  # noqa: E402

from test_aggregate_kernel_resources import AGG_KERNELS  # noqa: E402
from test_rows_kernel_resources import ROW_KERNELS  # noqa: E402
from test_where_kernel_resources import WHERE_KERNELS  # noqa: E402

GROUP_KERNELS = ["k_q_group_keys", "k_q_group_insert", "k_q_group_first", "k_q_group_tile_sums", "k_q_group_tile_apply", "k_q_group_emit",
                 "k_q_group_hist", "k_q_group_scan_sums", "k_q_group_scan_apply", "k_q_group_scatter", "k_q_group_bounds", "k_q_group_counts"]


@pytest.mark.parametrize("flags", [(), ("-DSJ_DEBUG_BOUNDS",)], ids=["product", "bounds-checked"])
def test_group_kernels_use_no_scratch(flags):
    rows = {}
    for name, vgprs, scratch, occ, lds in KR.kernels_of("query.hip", flags):
        rows.setdefault(name.split("(")[0].split("<")[0].split(" ")[-1], []).append((name, vgprs, scratch, occ, lds))
    neighbours = AGG_KERNELS + WHERE_KERNELS + ROW_KERNELS + ["k_q_count_path", "k_q_extract", "k_q_find_path", "k_q_col_len", "k_q_col_gather"]
    for kernel in GROUP_KERNELS + neighbours:
        assert len(rows.get(kernel, [])) == 1, (kernel, sorted(rows))
    assert sorted(k for k in rows if k.startswith("k_q_group_")) == sorted(GROUP_KERNELS)
    for kernel in GROUP_KERNELS + neighbours:
        for name, vgprs, scratch, occ, lds in rows[kernel]:
            print(name, "vgprs", vgprs, "scratch", scratch, "waves/SIMD", occ, "lds", lds)
            assert scratch == 0, (name, vgprs, scratch, occ, lds)
            assert occ >= 4, (name, vgprs, scratch, occ, lds)
