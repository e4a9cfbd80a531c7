"""The kernels of the ordering (sjhip_order_path, sjhip_order_path_strings and sjhip_order_paths: one pipeline, query.hip) exist
exactly once and there is no other of their family, those of the sort it shares with the grouping (sj_sort.h) once per key width
and for its two widths only, all stay off scratch and leave room for at least 4 waves per SIMD -- the bar
tests/test_group_kernel_resources.py sets for the grouping -- and the where kernels, whose second half the ordering shares, the row,
aggregate and group kernels named there keep that bar.  Compile-only: hipcc's resource remarks
(tools/kernel_resources.py), on the product and on the bounds-checked build."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as KR  # noqa: E402

from test_aggregate_kernel_resources import AGG_KERNELS  # noqa: E402
from test_group_kernel_resources import GROUP_KERNELS, SORT_KERNELS, check_sort_kernels  # noqa: E402
from test_rows_kernel_resources import ROW_KERNELS  # noqa: E402
from test_where_kernel_resources import WHERE_KERNELS  # noqa: E402

ORDER_KERNELS = ["k_q_order_init", "k_q_order_keys", "k_q_order_park", "k_q_order_chunks", "k_q_order_fold", "k_q_order_classes", "k_q_order_place",
                 "k_q_order_compact", "k_q_order_bounds", "k_q_order_rebuild", "k_q_order_flag", "k_q_order_flag_sums", "k_q_order_emit"]


@pytest.mark.parametrize("flags", [(), ("-DSJ_DEBUG_BOUNDS",)], ids=["product", "bounds-checked"])
def test_order_pipeline_kernels_use_no_scratch(flags):
    rows = {}
    for name, vgprs, scratch, occ, lds in KR.kernels_of("query.hip", flags):
        rows.setdefault(name.split("(")[0].split("<")[0].split(" ")[-1], []).append((name, vgprs, scratch, occ, lds))
    neighbours = WHERE_KERNELS + ROW_KERNELS + AGG_KERNELS + GROUP_KERNELS
    for kernel in ORDER_KERNELS + neighbours:
        assert len(rows.get(kernel, [])) == 1, (kernel, sorted(rows))
    assert sorted(k for k in rows if k.startswith("k_q_order_")) == sorted(ORDER_KERNELS)
    assert not [k for k in rows if k.startswith(("k_q_strord_", "k_q_mkord_"))]  # the families the pipeline replaced
    check_sort_kernels(rows)  # the sort as it was: unsigned int and unsigned long, no third width
    for kernel in ORDER_KERNELS + list(SORT_KERNELS) + neighbours:
        for name, vgprs, scratch, occ, lds in rows[kernel]:
            print(name, "vgprs", vgprs, "scratch", scratch, "waves/SIMD", occ, "lds", lds)
            assert scratch == 0, (name, vgprs, scratch, occ, lds)
            assert occ >= 4, (name, vgprs, scratch, occ, lds)
