"""The grouping by several keys (sjhip_group_paths, query.hip) has no kernels of its own: it runs the k_q_group_* kernels of
tests/test_group_kernel_resources.py, which keeps their list -- each exists exactly once, stays off scratch and leaves room for at
least 4 waves per SIMD --; the sort (sj_sort.h) is still instantiated for its two key widths only.  Compile-only: hipcc's resource remarks
(tools/kernel_resources.py), on the product and on the bounds-checked build."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as KR  # noqa: E402

from test_group_kernel_resources import GROUP_KERNELS, SORT_KERNELS, check_sort_kernels  # noqa: E402

SHARED_KERNELS = ["k_q_group_bounds", "k_q_group_counts", "k_q_agg_heads", "k_q_agg_rows", "k_q_agg_fold"]


@pytest.mark.parametrize("flags", [(), ("-DSJ_DEBUG_BOUNDS",)], ids=["product", "bounds-checked"])
def test_mkgrp_kernels_use_no_scratch(flags):
    rows = {}
    for name, vgprs, scratch, occ, lds in KR.kernels_of("query.hip", flags):
        rows.setdefault(name.split("(")[0].split("<")[0].split(" ")[-1], []).append((name, vgprs, scratch, occ, lds))
    for kernel in SHARED_KERNELS + GROUP_KERNELS:
        assert len(rows.get(kernel, [])) == 1, (kernel, sorted(rows))
    assert not [k for k in rows if k.startswith("k_q_mkgrp_")]  # one set of kernels: the single key's are the one-column case
    assert sorted(k for k in rows if k.startswith("k_q_group_")) == sorted(GROUP_KERNELS)
    check_sort_kernels(rows)  # the sort as it was: unsigned int and unsigned long, no third width
    for kernel in GROUP_KERNELS + SHARED_KERNELS + list(SORT_KERNELS):
        for name, vgprs, scratch, occ, lds in rows[kernel]:
            print(name, "vgprs", vgprs, "scratch", scratch, "waves/SIMD", occ, "lds", lds)
            assert scratch == 0, (name, vgprs, scratch, occ, lds)
            assert occ >= 4, (name, vgprs, scratch, occ, lds)
