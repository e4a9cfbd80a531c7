"""The kernels of the grouping by several keys (sjhip_group_paths, query.hip) exist exactly once, stay off scratch and leave room for
at least 4 waves per SIMD -- the bar of tests/test_group_kernel_resources.py, whose kernels the call shares and which keeps its
list; the sort (sj_sort.h) is still instantiated for its two key widths only.  Compile-only: hipcc's resource remarks
(tools/kernel_resources.py), on the product and on the bounds-checked build."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as KR  # noqa: E402

from test_group_kernel_resources import GROUP_KERNELS, SORT_KERNELS, check_sort_kernels  # noqa: E402

MKGRP_KERNELS = ["k_q_mkgrp_keys", "k_q_mkgrp_insert", "k_q_mkgrp_first", "k_q_mkgrp_tile_sums", "k_q_mkgrp_tile_apply", "k_q_mkgrp_emit"]
SHARED_KERNELS = ["k_q_group_bounds", "k_q_group_counts", "k_q_agg_heads", "k_q_agg_rows", "k_q_agg_fold"]


@pytest.mark.parametrize("flags", [(), ("-DSJ_DEBUG_BOUNDS",)], ids=["product", "bounds-checked"])
def test_mkgrp_kernels_use_no_scratch(flags):
    rows = {}
    for name, vgprs, scratch, occ, lds in KR.kernels_of("query.hip", flags):
        rows.setdefault(name.split("(")[0].split("<")[0].split(" ")[-1], []).append((name, vgprs, scratch, occ, lds))
    for kernel in MKGRP_KERNELS + SHARED_KERNELS + GROUP_KERNELS:
        assert len(rows.get(kernel, [])) == 1, (kernel, sorted(rows))
    assert sorted(k for k in rows if k.startswith("k_q_mkgrp_")) == sorted(MKGRP_KERNELS)
    assert sorted(k for k in rows if k.startswith("k_q_group_")) == sorted(GROUP_KERNELS)
    check_sort_kernels(rows)  # the sort as it was: unsigned int and unsigned long, no third width
    for kernel in MKGRP_KERNELS + SHARED_KERNELS + list(SORT_KERNELS):
        for name, vgprs, scratch, occ, lds in rows[kernel]:
            print(name, "vgprs", vgprs, "scratch", scratch, "waves/SIMD", occ, "lds", lds)
            assert scratch == 0, (name, vgprs, scratch, occ, lds)
            assert occ >= 4, (name, vgprs, scratch, occ, lds)
