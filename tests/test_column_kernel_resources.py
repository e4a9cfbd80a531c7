"""The column kernels of query.hip (sjhip_extract_path / sjhip_extract_path_strings) exist and stay off scratch: k_q_col_len and
k_q_col_gather carry the float formatter of sj_ftoa.h, which once spilled in MarshalJSON (tests/test_kernel_resources.py).
Compile-only: hipcc's resource remarks (tools/kernel_resources.py), on the product and on the bounds-checked build."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as KR  # noqa: E402

COLUMN_KERNELS = ("k_q_extract", "k_q_col_len", "k_q_col_tile_sums", "k_q_col_tile_apply", "k_q_col_gather")


@pytest.mark.parametrize("flags", [(), ("-DSJ_DEBUG_BOUNDS",)], ids=["product", "bounds-checked"])
def test_column_kernels_use_no_scratch(flags):
    rows = {name.split("(")[0]: (vgprs, scratch, occ) for name, vgprs, scratch, occ, lds in KR.kernels_of("query.hip", flags)}
    for k in COLUMN_KERNELS:
        assert k in rows, (k, sorted(rows))
        assert rows[k][1] == 0, (k, rows[k])
        assert rows[k][2] >= 4, (k, rows[k])  # (at least half the waves per SIMD: the one-lane-per-record walks hide latency)
