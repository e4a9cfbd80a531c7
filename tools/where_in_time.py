"""The set predicate (where_path_in) on 1 M rows, next to what a caller had before -- where_paths with one EQ per value under OR
(up to 16 values), or the key column fetched and numpy.isin on the host -- and next to where_path with ONE EQ_STRING on the same
rows, which is the walk and the narrowing without any set:
python tools/where_in_time.py

The document of tools/where_time.py: configs[4], parking-citations x1000 ND, 1 M records, no selection.  The query is Make IN a
set of 16, 1 024 and 65 536 values.  The sets are the most frequent makes of the document, taken from the largest down while they
cover at most half of the rows, then makes that do not occur ("ZZ" + a number) up to the set's size: about half of the rows match
whatever the size, and every row that does not match probes to an empty slot.
  (a) where_path_in per set size, against where_path with one EQ_STRING, and the count calls of both (no narrowing: the walk, the
      upload and build of the set, the probe)
  (b) the set of 16 against where_paths with 16 tests under OR
  (c) the host route: the Make column fetched (extract_path_strings), numpy.isin on the host -- and then no call takes the mask
The selection is put back before every timed call (select_records: not timed).

Host wall time of warmed calls; every call ends in a synchronisation.  Median of REPS runs, three medians each."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "simdjson-go_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402  (initialises its HIP runtime first, tests/conftest.py)

import sjhip  # noqa: E402
import workloads  # noqa: E402

REPS = 11
SIZES = (16, 1024, 65536)


def med(fn, setup=None, reps=REPS):
    """median wall time of fn() in ms; setup() runs before every call and is not timed"""
    ts = []
    for k in range(reps + 2):
        if setup:
            setup()
        t0 = time.perf_counter()
        fn()
        if k >= 2:
            ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1e3


def three(fn, setup=None, reps=REPS):
    ms = [med(fn, setup, reps) for _ in range(3)]
    return statistics.median(ms), " ".join("%.3f" % x for x in ms)


def large_strings(values):
    """Arrow's large-string layout of a list of bytes: what where_path_in takes as (offsets, data)"""
    off = np.zeros(len(values) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(v) for v in values])
    return off, np.frombuffer(b"".join(values), dtype=np.uint8)


def host_isin(off, data, values):
    """the fetched string column as fixed-width bytes, then numpy.isin: the mask a caller builds on the host"""
    lens = np.diff(off.astype(np.int64))
    width = max(int(lens.max()), max(len(v) for v in values))
    rows = np.repeat(np.arange(len(lens)), lens)
    cols = np.arange(int(lens.sum())) - np.repeat(off[:-1].astype(np.int64), lens)
    fixed = np.zeros((len(lens), width), dtype=np.uint8)
    fixed[rows, cols] = np.frombuffer(data, dtype=np.uint8)[:len(rows)]
    keys = fixed.view("S%d" % width).ravel()
    return np.isin(keys, np.array(values, dtype="S%d" % width))


def main():
    ctx = sjhip.Context(0)
    S = ctx.COL_STRING
    doc = workloads.c5_parking_nd(1000).rstrip(b"\n")
    d = torch.empty(len(doc) + 256, dtype=torch.uint8, device="cuda:0")
    d[:len(doc)].copy_(torch.frombuffer(bytearray(doc), dtype=torch.uint8))
    torch.cuda.synchronize()
    tl, sl = ctx.parse_device(d.data_ptr(), len(doc), ndjson=True, copy_strings=True)
    back = ctx.select_records
    path = (b"Make",)
    g = ctx.group_path(path, S)
    rows = g.rows
    print(f"# {torch.cuda.get_device_name(0)}; host wall time in ms, median of {REPS} warmed calls (three medians), device-resident result")
    print(f"parking: {len(doc)} B, tape {tl} words, {rows} rows, {g.groups} distinct makes")
    real, covered = [], 0
    for j in np.argsort(-g.group_rows.astype(np.int64), kind="stable"):
        if covered + int(g.group_rows[j]) <= rows // 2 and len(real) < 16:
            real.append(g.keys[j])
            covered += int(g.group_rows[j])
    sets = {n: real + [b"ZZ%06d" % k for k in range(n - len(real))] for n in SIZES}
    print(f"the sets: {len(real)} makes of the document ({covered} rows, {100.0 * covered / rows:.1f} %) and makes that do not occur, up to {SIZES}")

    back()
    eq = (path, ctx.OP_EQ_STRING, real[0])
    w1, t1 = three(lambda: ctx.where_path(*eq), back)
    c1, u1 = three(lambda: ctx.count_where_path(*eq))
    print("  (a) per set size, beside one EQ_STRING on the same rows")
    print(f"      where_path, one EQ_STRING                 {w1:8.3f} ms  (medians {t1})")
    print(f"      count_where_path, one EQ_STRING           {c1:8.3f} ms  (medians {u1})")
    for n in SIZES:
        arrow = large_strings(sets[n])
        back()
        kept = ctx.where_path_in(path, S, arrow)
        back()
        assert kept == (rows, covered) and ctx.count_where_path_in(path, S, arrow) == covered
        wn, tn = three(lambda: ctx.where_path_in(path, S, arrow), back)
        cn, un = three(lambda: ctx.count_where_path_in(path, S, arrow))
        print(f"      where_path_in, {n:6d} values             {wn:8.3f} ms  (medians {tn})   / where_path {wn / w1:5.2f}   {covered} rows kept")
        print(f"      count_where_path_in, {n:6d} values       {cn:8.3f} ms  (medians {un})   / count_where_path {cn / c1:5.2f}")
        print(f"          the set: {int(arrow[0][-1]) + 8 * (n + 1)} bytes uploaded, a table of {4 * max(64, 1 << (2 * n - 1).bit_length())} bytes")

    preds = [(path, ctx.OP_EQ_STRING, v) for v in sets[16]]
    program = bytes([0] + [x for p in range(1, 16) for x in (p, ctx.WHERE_OR)])
    back()
    assert ctx.where_paths(preds, program) == (rows, covered)
    arrow = large_strings(sets[16])
    m16, t16 = three(lambda: ctx.where_paths(preds, program), back)
    i16, u16 = three(lambda: ctx.where_path_in(path, S, arrow), back)
    print("  (b) the set of 16")
    print(f"      where_paths, 16 tests under OR            {m16:8.3f} ms  (medians {t16})")
    print(f"      where_path_in, 16 values                  {i16:8.3f} ms  (medians {u16})   16 ORs / IN {m16 / i16:5.2f}")

    back()
    print("  (c) the host route: the Make column fetched, numpy.isin (and no call takes the mask back)")
    for n in SIZES:
        def masked():
            off, data, st = ctx.extract_path_strings(path)
            return int(host_isin(off, data, sets[n]).sum())

        assert masked() == covered
        mh, th = three(masked, reps=5)
        print(f"      column fetch + isin, {n:6d} values       {mh:8.3f} ms  (medians {th})")
    fetch, tf = three(lambda: ctx.extract_path_strings(path), reps=5)
    print(f"      the column fetch alone                    {fetch:8.3f} ms  (medians {tf})")
    del d
    ctx.close()


if __name__ == "__main__":
    main()
