"""The kernels of the row schema (sjhip_row_schema; query.hip) exist exactly as listed -- the status count, the keys, the insert
behind its election, the first-occurrence flags, the two tile steps of their scan, the emit, the bounds and the counts --, stay
off scratch and leave room for at least 4 waves per SIMD: the bar of the member kernels, whose walk they follow.  Compile-only:
hipcc's resource remarks (tools/kernel_resources.py), on the product and on the bounds-checked build."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as KR  # noqa: E402

SCHEMA_KERNELS = ["k_q_schema_status", "k_q_schema_keys", "k_q_schema_insert", "k_q_schema_first", "k_q_schema_tile_sums",
                  "k_q_schema_tile_apply", "k_q_schema_emit", "k_q_schema_bounds", "k_q_schema_counts"]


@pytest.mark.parametrize("flags", [(), ("-DSJ_DEBUG_BOUNDS",)], ids=["product", "bounds-checked"])
def test_schema_kernels_use_no_scratch(flags):
    rows = {}
    for name, vgprs, scratch, occ, lds in KR.kernels_of("query.hip", flags):
        rows.setdefault(name.split("(")[0].split("<")[0].split(" ")[-1], []).append((name, vgprs, scratch, occ, lds))
    assert sorted(k for k in rows if k.startswith("k_q_schema_")) == sorted(SCHEMA_KERNELS)
    for kernel in SCHEMA_KERNELS:
        assert len(rows[kernel]) == 1, (kernel, rows[kernel])
        for name, vgprs, scratch, occ, lds in rows[kernel]:
            print(name, "vgprs", vgprs, "scratch", scratch, "waves/SIMD", occ, "lds", lds)
            assert scratch == 0, (name, vgprs, scratch, occ, lds)
            assert occ >= 4, (name, vgprs, scratch, occ, lds)
