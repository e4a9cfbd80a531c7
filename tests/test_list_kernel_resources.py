"""The list-column kernels of query.hip (sjhip_extract_path_list / sjhip_extract_path_list_strings) exist and stay off scratch: the
measure and gather kernels of Array.AsStringCvt carry the float formatter of sj_ftoa.h next to the wave loops over long arrays and
long strings.  Compile-only: hipcc's resource remarks (tools/kernel_resources.py), on the product and on the bounds-checked build;
the occupancy floor is the one tests/test_column_kernel_resources.py demands of the other walk kernels."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as KR  # noqa: E402

LIST_KERNELS = ("k_q_list_measure", "k_q_list_measure_cvt", "k_q_list_tile_sums", "k_q_list_tile_apply", "k_q_list_gather_num",
                "k_q_list_gather_str", "k_q_list_gather_cvt")


@pytest.mark.parametrize("flags", [(), ("-DSJ_DEBUG_BOUNDS",)], ids=["product", "bounds-checked"])
def test_list_kernels_use_no_scratch(flags):
    rows = {name.split("(")[0]: (vgprs, scratch, occ) for name, vgprs, scratch, occ, lds in KR.kernels_of("query.hip", flags)}
    for k in LIST_KERNELS:
        assert k in rows, (k, sorted(rows))
        assert rows[k][1] == 0, (k, rows[k])
        assert rows[k][2] >= 4, (k, rows[k])
