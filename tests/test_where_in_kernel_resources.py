"""The kernels of the set predicate (sjhip_where_path_in / sjhip_count_where_path_in, query.hip) -- k_q_in_build, one lane per value
of the set, and k_q_in_mark, one lane per row, of which the count is a branch and not a second kernel -- stay off scratch, and
their occupancy is not below that of k_q_where_mark, the mark of the single predicate whose place k_q_in_mark takes.  Compile-only:
hipcc's resource remarks (tools/kernel_resources.py), on the product and on the bounds-checked build."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as KR  # noqa: E402


@pytest.mark.parametrize("flags", [(), ("-DSJ_DEBUG_BOUNDS",)], ids=["product", "bounds-checked"])
def test_in_kernels_use_no_scratch_and_keep_the_occupancy_of_where_mark(flags):
    found = {}
    for name, vgprs, scratch, occ, lds in KR.kernels_of("query.hip", flags):
        found.setdefault(name.split("(")[0].split("<")[0], []).append((vgprs, scratch, occ, lds))
    for kernel in ("k_q_in_build", "k_q_in_mark", "k_q_where_mark"):
        assert len(found.get(kernel, [])) == 1, (kernel, found.get(kernel))
    occ_where = found["k_q_where_mark"][0][2]
    for kernel in ("k_q_in_build", "k_q_in_mark"):
        vgprs, scratch, occ, lds = found[kernel][0]
        assert scratch == 0, (kernel, found[kernel])
        assert occ >= occ_where, (kernel, found[kernel], occ_where)
        assert lds == 0, (kernel, found[kernel])
