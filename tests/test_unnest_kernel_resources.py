"""The kernels of the unnest (sjhip_unnest_rows, query.hip) exist -- one lane pass over the parents, the count and the write
instantiation of the tile pass, the parent offsets --, stay off scratch -- the tile pass keeps its eight words, its masks and the
parents of its starts in registers -- and leave room for at least 4 waves per SIMD; the row kernels, whose depth passes and
classification the unnest shares, keep that bar.  Compile-only: hipcc's resource remarks (tools/kernel_resources.py), on the
product and on the bounds-checked build."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as KR  # noqa: E402

from test_rows_kernel_resources import ROW_KERNELS  # noqa: E402

UNNEST_KERNELS = ["k_q_unnest_parents", "k_q_unnest_offsets"]


@pytest.mark.parametrize("flags", [(), ("-DSJ_DEBUG_BOUNDS",)], ids=["product", "bounds-checked"])
def test_unnest_kernels_use_no_scratch(flags):
    rows = {}
    for name, vgprs, scratch, occ, lds in KR.kernels_of("query.hip", flags):
        rows.setdefault(name.split("(")[0].split("<")[0].split(" ")[-1], []).append((name, vgprs, scratch, occ, lds))
    for kernel in UNNEST_KERNELS + ROW_KERNELS:
        assert len(rows.get(kernel, [])) == 1, (kernel, sorted(rows))
    assert len(rows.get("k_q_unnest_tile", [])) == 2, sorted(rows)  # the count, the write
    assert len(rows.get("k_q_rows_tile", [])) == 3, sorted(rows)
    assert sorted(k for k in rows if k.startswith("k_q_unnest_")) == sorted(UNNEST_KERNELS + ["k_q_unnest_tile"])
    for kernel in UNNEST_KERNELS + ["k_q_unnest_tile"] + ROW_KERNELS + ["k_q_rows_tile"]:
        for name, vgprs, scratch, occ, lds in rows[kernel]:
            print(name, "vgprs", vgprs, "scratch", scratch, "waves/SIMD", occ, "lds", lds)
            assert scratch == 0, (name, vgprs, scratch, occ, lds)
            assert occ >= 4, (name, vgprs, scratch, occ, lds)
