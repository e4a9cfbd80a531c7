"""Order rows by two keys on the device-resident tape, next to the host route a caller had before:
python tools/order_multi_time.py [few] [unique] [parking] [--out DIR]

Three documents of 1 M rows, ND, no selection (the rows are the records):
  few      synthetic {"a":..,"b":..}: a has 50 distinct values, b is a random int64 -- every row reaches column 1, in 50 classes
  unique   the same with a drawn from 10 M values: about 5 % of the rows tie on a and reach column 1
  parking  configs[4]: parking-citations x1000 ND, keys (Make, Color): two short string keys with many duplicates
The order is (first key ascending, second key descending) on the synthetic documents, both ascending on parking.  For each,
alternating on the same device:
  (a) order_paths(two keys, limit=10) + marshal_rows, fetched     "the first 10", as text, and nothing else over PCIe
  (b) order_paths(two keys, limit=0), fetched                     the full ORDER BY: order and status of every row
  (c) extract_table of both key columns, fetched, + numpy.lexsort the route of the parent commit (which has no way back to the
      device with the row numbers it found); a string column becomes codes through numpy.unique over fixed-width byte strings
and the single-key pair: order_paths with the first key alone against order_path / order_path_strings on the same rows.
Host wall time of warmed calls; every call ends in a synchronisation.  Median of REPS runs, three medians each.  The output is
also written to DIR/rNN_order_multi_time.txt (DIR: profiles/ of the repository), NN the next free number."""
import os
import random
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = sys.argv[1:]
sys.path[:0] = [os.path.join(ROOT, "simdjson-go_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402  (initialises its HIP runtime first, tests/conftest.py)

import sjhip  # noqa: E402
import workloads  # noqa: E402

REPS = 7
N = 1000000
LINES = []
I, S = sjhip.Context.COL_INT, sjhip.Context.COL_STRING


def say(text):
    print(text, flush=True)
    LINES.append(text)


def med(fn, reps=REPS):
    """median wall time of fn() in ms"""
    ts = []
    for k in range(reps + 2):
        t0 = time.perf_counter()
        fn()
        if k >= 2:
            ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1e3


def resident(ctx, doc):
    d = torch.empty(len(doc) + 256, dtype=torch.uint8, device="cuda:0")
    d[:len(doc)].copy_(torch.frombuffer(bytearray(doc), dtype=torch.uint8))
    torch.cuda.synchronize()
    return d, ctx.parse_device(d.data_ptr(), len(doc), ndjson=True, copy_strings=True)


def document(name):
    """-> (the document, [(path, kind, descending)] x 2)"""
    if name == "parking":
        return workloads.c5_parking_nd(1000).rstrip(b"\n"), [((b"Make",), S, False), ((b"Color",), S, False)]
    rnd = random.Random(24)
    distinct = 50 if name == "few" else 10000000
    lines = ['{"a":%d,"b":%d}' % (rnd.randrange(distinct), rnd.randrange(-1 << 63, 1 << 63)) for _ in range(N)]
    return "\n".join(lines).encode(), [((b"a",), I, False), ((b"b",), I, True)]


def codes(column):
    """a string column as fetched -> the rank of every row's key among the distinct keys"""
    off, data, st = column
    off = off.astype(np.int64)
    lens = np.diff(off)
    width = max(int(lens.max()), 1)
    mat = np.zeros((len(lens), width), dtype=np.uint8)
    raw = np.frombuffer(data, dtype=np.uint8)
    row = np.repeat(np.arange(len(lens)), lens)
    mat[row, np.arange(len(raw)) - np.repeat(off[:-1], lens)] = raw
    keys = mat.view("S%d" % width).ravel()  # (no key of these documents holds a NUL byte, which this dtype would strip)
    return np.unique(keys, return_inverse=True)[1].astype(np.int64)


def host_sort(table, cols):
    """the row numbers in rank order: numpy.lexsort, its last key the primary one; per column "has no OK key" in front of the key (a
    row without one holds 0 or the empty string, so such rows tie)"""
    keys = []
    for column, (_, kind, desc) in zip(table, cols):
        k = codes(column) if kind == S else column[0]
        keys += [column[-1] != 0, ~k if desc else k]  # (the complement reverses an int64 without overflow)
    return np.lexsort(keys[::-1])


def main():
    ctx = sjhip.Context(0)
    names = [a for a in ARGS if a in ("few", "unique", "parking")] or ["few", "unique", "parking"]
    out_dir = ARGS[ARGS.index("--out") + 1] if "--out" in ARGS else os.path.join(ROOT, "profiles")
    say(f"# {torch.cuda.get_device_name(0)}; host wall time in ms, median of {REPS} warmed calls, device-resident result, 1 M rows")
    for name in names:
        doc, cols = document(name)
        d, (tl, sl) = resident(ctx, doc)
        plain = [(path, kind) for path, kind, _ in cols]
        first = cols[0]

        def top10():
            ctx.select_records()
            o = ctx.order_paths(cols, limit=10)
            return o, ctx.marshal_rows(offsets=True)

        def full():
            ctx.select_records()
            return ctx.order_paths(cols)

        def full_device_only():
            ctx.select_records()
            return ctx.order_paths(cols, fetch=False)

        def host():
            table = ctx.extract_table(plain)
            return table, host_sort(table, cols)

        def one_multi():
            ctx.select_records()
            return ctx.order_paths([first])

        def one_single():
            ctx.select_records()
            if first[1] == S:
                return ctx.order_path_strings(first[0], descending=first[2])
            return ctx.order_path(first[0], first[1], descending=first[2])

        o = full()
        table, perm = host()
        assert o.rows == len(perm) and np.array_equal(o.order.astype(np.int64), perm)
        top, (n10, text, _) = top10()
        assert top.rows == 10 == n10
        assert np.array_equal(one_multi().order, one_single().order)
        counts = np.unique(codes(table[0]) if first[1] == S else table[0][0], return_counts=True)[1]
        tied = int(counts[counts > 1].sum())
        runs = {"a": [], "b": [], "n": [], "c": [], "e": [], "m1": [], "s1": []}
        for _ in range(3):  # alternating
            runs["a"].append(med(top10))
            runs["b"].append(med(full))
            runs["n"].append(med(full_device_only))
            runs["c"].append(med(host, reps=3))
            runs["e"].append(med(lambda: ctx.extract_table(plain), reps=3))
            runs["m1"].append(med(one_multi))
            runs["s1"].append(med(one_single))
        ctx.select_records()
        m = {k: statistics.median(v) for k, v in runs.items()}
        show = lambda k: " ".join("%.3f" % x for x in runs[k])  # noqa: E731
        n = len(perm)
        what = ", ".join("%s %s" % (b".".join(path).decode(), "desc" if desc else "asc") for path, _, desc in cols)
        say(f"{name}: {len(doc)} B, tape {tl} words, {n} rows, keys ({what}), {len(counts)} distinct first keys, {tied} rows tie on the first key")
        say(f"  (a) order_paths(limit=10) + marshal_rows             {m['a']:10.3f} ms  (medians {show('a')})   PCIe {90 + len(text) + 88} B")
        say(f"  (b) order_paths(limit=0), fetched                    {m['b']:10.3f} ms  (medians {show('b')})   PCIe {9 * n} B")
        say(f"      order_paths(limit=0), not fetched                {m['n']:10.3f} ms  (medians {show('n')})")
        say(f"  (c) extract_table fetched + numpy.lexsort            {m['c']:10.3f} ms  (medians {show('c')})   (c)/(a) {m['c'] / m['a']:6.2f}  (c)/(b) {m['c'] / m['b']:6.2f}")
        say(f"      extract_table fetched, not sorted                {m['e']:10.3f} ms  (medians {show('e')})")
        say(f"  one key: order_paths([first]), fetched               {m['m1']:10.3f} ms  (medians {show('m1')})")
        say(f"  one key: order_path / order_path_strings, fetched    {m['s1']:10.3f} ms  (medians {show('s1')})   order_paths / single {m['m1'] / m['s1']:5.2f}")
        del d
    ctx.close()
    os.makedirs(out_dir, exist_ok=True)
    taken = [int(x.group(1)) for x in (re.match(r"r(\d+)", f) for f in os.listdir(out_dir)) if x]
    path = os.path.join(out_dir, "r%02d_order_multi_time.txt" % (max(taken, default=0) + 1))
    with open(path, "w") as f:
        f.write("\n".join(LINES) + "\n")
    print("written to", path)


if __name__ == "__main__":
    main()
