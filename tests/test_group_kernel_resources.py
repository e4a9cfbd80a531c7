"""The kernels of the grouping (sjhip_group_path, query.hip) exist exactly once, those of the sort it shares with the ordering
(sj_sort.h) once per key width, all stay off scratch and leave room for at least 4 waves per SIMD -- the bar
tests/test_aggregate_kernel_resources.py sets for the aggregates -- and the aggregate kernels, which took the row permutation of the
grouping, and the neighbours named there keep that bar.  Compile-only: hipcc's resource remarks (tools/kernel_resources.py), on the
product and on the bounds-checked build."""
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
                 "k_q_group_bounds", "k_q_group_counts"]
# the radix sort of the grouping and the ordering: how often each kernel exists (the templated ones: uint32 and uint64 keys)
SORT_KERNELS = {"k_q_sort_hist": 2, "k_q_sort_scatter": 2, "k_q_sort_scan_sums": 1, "k_q_sort_scan_apply": 1}


def check_sort_kernels(rows):
    """rows: {kernel name without template arguments: [(name, vgprs, scratch, occ, lds)]} of query.hip"""
    for kernel, copies in SORT_KERNELS.items():
        assert len(rows.get(kernel, [])) == copies, (kernel, sorted(rows))
    assert sorted(k for k in rows if k.startswith("k_q_sort_")) == sorted(SORT_KERNELS)
    keys = sorted(name.split("<")[1].split(">")[0] for kernel in ("k_q_sort_hist", "k_q_sort_scatter") for name, *_ in rows[kernel])
    assert keys == ["unsigned int", "unsigned int", "unsigned long", "unsigned long"], keys


@pytest.mark.parametrize("flags", [(), ("-DSJ_DEBUG_BOUNDS",)], ids=["product", "bounds-checked"])
def test_group_kernels_use_no_scratch(flags):
    rows = {}
    for name, vgprs, scratch, occ, lds in KR.kernels_of("query.hip", flags):
        rows.setdefault(name.split("(")[0].split("<")[0].split(" ")[-1], []).append((name, vgprs, scratch, occ, lds))
    neighbours = AGG_KERNELS + WHERE_KERNELS + ROW_KERNELS + ["k_q_count_path", "k_q_extract", "k_q_find_path", "k_q_col_len", "k_q_col_gather"]
    for kernel in GROUP_KERNELS + neighbours:
        assert len(rows.get(kernel, [])) == 1, (kernel, sorted(rows))
    assert sorted(k for k in rows if k.startswith("k_q_group_")) == sorted(GROUP_KERNELS)
    check_sort_kernels(rows)
    for kernel in GROUP_KERNELS + list(SORT_KERNELS) + neighbours:
        for name, vgprs, scratch, occ, lds in rows[kernel]:
            print(name, "vgprs", vgprs, "scratch", scratch, "waves/SIMD", occ, "lds", lds)
            assert scratch == 0, (name, vgprs, scratch, occ, lds)
            assert occ >= 4, (name, vgprs, scratch, occ, lds)
