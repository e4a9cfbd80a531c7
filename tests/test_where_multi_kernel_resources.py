"""The mark kernel of the row predicates over several tests (sjhip_where_paths / sjhip_count_where_paths, query.hip) exists exactly
once -- the count is a branch of it, not a second kernel --, stays off scratch -- the truth of the predicates is a mask, the stack
of the program the bits of one register, the resume stack of the walk LDS -- and leaves room for at least 4 waves per SIMD beside
its 32 KiB of LDS per block.  Compile-only: hipcc's resource remarks (tools/kernel_resources.py), on the product and on the
bounds-checked build."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as KR  # noqa: E402


@pytest.mark.parametrize("flags", [(), ("-DSJ_DEBUG_BOUNDS",)], ids=["product", "bounds-checked"])
def test_where_multi_mark_uses_no_scratch(flags):
    found = [(vgprs, scratch, occ, lds) for name, vgprs, scratch, occ, lds in KR.kernels_of("query.hip", flags)
             if name.split("(")[0].split("<")[0] == "k_q_where_multi_mark"]
    assert len(found) == 1, found
    vgprs, scratch, occ, lds = found[0]
    assert scratch == 0, found[0]
    assert occ >= 4, found[0]  # (the one-lane-per-row walk hides its latency behind other waves)
    assert lds == 2 * 16 * 4 * 256, found[0]  # the resume stack: two u32 for each of 16 levels and 256 lanes
