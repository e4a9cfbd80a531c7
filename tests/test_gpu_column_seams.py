"""GPU: the string column and the list columns on the cuts of their kernels -- COL_SHORT, LIST_SHORT, the 64-byte and 64-element
wave steps, the first failing element of a step, the wait-and-copy rounds, AsString's carried base, the lanes without a record,
entry n and the scan tiles of n + 1 entries.  The cases are those of tests/col_geometry.py (tests/test_col_geometry.py shows on
the CPU that each lies on the cut it is named for and which of them tells which mutated kernel from the real one).  Every case is
extracted in every mode of its family, in both copy modes, and its list offsets, string offsets, bytes, value bits, statuses
and the totals the extraction reports are compared exactly with the builder's own expectation and, through the checkers of
tests/test_gpu_columns.py and tests/test_gpu_lists.py, with the walkers over the oracle's parse."""
import numpy as np
import pytest

import col_geometry as G
from test_gpu_columns import check_strings as check_string_column
from test_gpu_lists import check_numbers as check_number_lists, check_strings as check_string_lists
from test_gpu_parse import ctx  # noqa: F401

pytestmark = pytest.mark.gpu


def same(got, want, what):
    assert got.dtype == np.uint64 and np.array_equal(got, np.array(want, dtype=np.uint64)), what


def run_strings(ctx, case, checked=False):
    """checked: follow every fetch with a query call that ends in the bounds check (the column's own fetch does not)"""
    for cvt, mode in zip((False, True), G.MODES["strings"]):
        want = G.expect(case, mode)
        nr, nb = ctx.extract_path_strings(case.path, cvt=cvt, fetch=False)
        assert (nr, nb) == want["totals"], (case.name, mode)
        off, data, st = ctx.fetch_path_strings(nr, nb)
        if checked:
            ctx.count_where_path(case.path, ctx.OP_EXISTS)
        assert st.tolist() == want["status"], (case.name, mode)
        same(off, want["off"], (case.name, mode))
        assert data == want["data"], (case.name, mode)


def run_numbers(ctx, case):
    for mode, kind in G.KIND.items():
        want = G.expect(case, mode)
        nr, ne = ctx.extract_path_list(case.path, kind, fetch=False)
        assert (nr, ne) == want["totals"], (case.name, mode)
        off, vals, st = ctx.fetch_path_list(nr, ne, kind)
        assert st.tolist() == want["status"], (case.name, mode)
        same(off, want["off"], (case.name, mode))
        same(vals.view(np.uint64), want["vals"], (case.name, mode))


def run_list_strings(ctx, case):
    for cvt, mode in zip((False, True), G.MODES["list_strings"]):
        want = G.expect(case, mode)
        nr, ne, nb = ctx.extract_path_list_strings(case.path, cvt=cvt, fetch=False)
        assert (nr, ne, nb) == want["totals"], (case.name, mode)
        off, soff, data, st = ctx.fetch_path_list_strings(nr, ne, nb)
        assert st.tolist() == want["status"], (case.name, mode)
        same(off, want["off"], (case.name, mode))
        same(soff, want["soff"], (case.name, mode))
        assert data == want["data"], (case.name, mode)


RUN = {"strings": run_strings, "numbers": run_numbers, "list_strings": run_list_strings}
WALKERS = {"strings": check_string_column, "numbers": check_number_lists, "list_strings": check_string_lists}


def run_case(ctx, case, **kw):
    for copy in (True, False):
        ctx.parse(case.doc, ndjson=True, copy_strings=copy)
        if case.select is not None:
            assert ctx.select_rows(case.select) == (1, len(case.rows))
        RUN[case.family](ctx, case, **kw)
        WALKERS[case.family](ctx, G.walk(case.doc, copy, case.select), case.path)
        if case.select is not None:
            ctx.select_records()


@pytest.mark.parametrize("case", G.string_cases(), ids=lambda c: c.name)
def test_string_column(ctx, case):
    run_case(ctx, case)


@pytest.mark.parametrize("case", G.number_cases(), ids=lambda c: c.name)
def test_number_lists(ctx, case):
    run_case(ctx, case)


@pytest.mark.parametrize("case", G.list_string_cases(), ids=lambda c: c.name)
def test_string_lists(ctx, case):
    run_case(ctx, case)
