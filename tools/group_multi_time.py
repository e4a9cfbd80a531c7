"""Group rows by two keys with two aggregates on the device-resident tape, next to the host route a caller had before:
python tools/group_multi_time.py [synthetic] [parking] [--out DIR]

Two documents of 1 M rows, ND, no selection (the rows are the records):
  synthetic  {"a":"m<0..59>","b":<0..16>,"v":<int>,"w":<quarters>}: 60 x 17 tuples, numeric values (every float sum exact)
  parking    configs[4]: parking-citations x1000 ND, keys (Make, Color), values sum(Fine) FLOAT and max(IssueTime) INT -- the file
             spells both as strings, so every value is not_ok there and the reduction only counts; the key side is the real one
For each, alternating on the same device:
  (a) group_paths(two keys, two values), fetched          keys, key_ok and aggregates per group, codes and statuses per row
  (b) group_paths(two keys, two values), not fetched      the build alone
  (c) extract_table of the four columns, fetched, + numpy the route of the parent commit: string columns become codes through
      numpy.unique over fixed-width byte strings, the tuple through one more numpy.unique, the aggregates through numpy.bincount
      and ufunc.at
  (d) two group_path calls on the first key, one per value: what a second aggregate cost before
and the one-column pair, fetched: group_paths([first key], [first value]) against group_path(first key, first value) -- the
single-key call is the parent commit's code, unchanged.  Before anything is timed (a) is checked against (c) -- groups, first_row,
group_rows, codes, count, not_ok, sums, min, max -- and the one-column pair against each other, bit for bit.
The spread comes first: SPREAD_RUNS medians of group_path alone, alternating with the other calls; its spread is max - min of
those medians, and the one-column result is the difference of the two medians of medians, judged against it.
Host wall time of warmed calls; every call ends in a synchronisation.  Median of REPS runs.  The output is also written to
DIR/rNN_group_multi_time.txt (DIR: profiles/ of the repository), NN the next free number of profiles/."""
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
SPREAD_RUNS = 9
N = 1000000
LINES = []
F, I, S = sjhip.Context.COL_FLOAT, sjhip.Context.COL_INT, sjhip.Context.COL_STRING
DT = {F: np.float64, I: np.int64}


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


def document(name, n=N):
    """-> (the document, key columns, value columns)"""
    if name == "parking":
        doc = workloads.c5_parking_nd(max(n // 1000, 1)).rstrip(b"\n")
        return doc, [((b"Make",), S), ((b"Color",), S)], [((b"Fine",), F), ((b"IssueTime",), I)]
    rnd = random.Random(25)
    lines = ['{"a":"m%d","b":%d,"v":%d,"w":%d.%s}' % (rnd.randrange(60), rnd.randrange(17), rnd.randrange(-1000, 1000), rnd.randrange(1000),
                                                       rnd.choice(("0", "25", "5", "75"))) for _ in range(n)]
    return "\n".join(lines).encode(), [((b"a",), S), ((b"b",), I)], [((b"v",), I), ((b"w",), F)]


def codes(column, kind):
    """a key column as fetched -> a small integer per row, equal for equal keys"""
    if kind != S:
        return np.unique(column[0], return_inverse=True)[1].astype(np.int64)
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


def host_group(table, kcols, vcols):
    """the grouping of the fetched table: -> (codes per row with -1 for a row in no group, first_row, group_rows,
    [(count, not_ok, sum, min, max) per value column]); groups numbered by first occurrence"""
    nk = len(kcols)
    ok = np.ones(len(table[0][-1]), dtype=bool)
    tup = np.zeros(len(ok), dtype=np.int64)
    for column, (_, kind) in zip(table[:nk], kcols):
        c = codes(column, kind)
        ok &= column[-1] == 0
        tup = tup * (int(c.max()) + 1) + c
    rows = np.flatnonzero(ok)
    _, first, inv = np.unique(tup[rows], return_index=True, return_inverse=True)
    rank = np.empty(len(first), dtype=np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(len(first))  # the unique tuples renumbered by their first row
    g = rank[inv]
    G = len(first)
    out_codes = np.full(len(ok), -1, dtype=np.int64)
    out_codes[rows] = g
    first_row = np.sort(rows[first])
    group_rows = np.bincount(g, minlength=G)
    aggs = []
    for column, (_, kind) in zip(table[nk:], vcols):
        vals, st = column[0][rows], column[-1][rows] == 0
        count = np.bincount(g[st], minlength=G)
        total = np.zeros(G, dtype=DT[kind])
        np.add.at(total, g[st], vals[st])
        lo, hi = np.zeros(G, dtype=DT[kind]), np.zeros(G, dtype=DT[kind])
        if st.any():
            big = np.inf if kind == F else np.iinfo(np.int64).max
            lo2, hi2 = np.full(G, big, dtype=DT[kind]), np.full(G, -big, dtype=DT[kind])
            np.minimum.at(lo2, g[st], vals[st])
            np.maximum.at(hi2, g[st], vals[st])
            lo[count > 0], hi[count > 0] = lo2[count > 0], hi2[count > 0]
        aggs.append((count, group_rows - count, total, lo, hi))
    return out_codes, first_row, group_rows, aggs


def check(got, want):
    wcodes, first_row, group_rows, aggs = want
    assert got.groups == len(first_row), (got.groups, len(first_row))
    assert np.array_equal(got.first_row.astype(np.int64), first_row) and np.array_equal(got.group_rows.astype(np.int64), group_rows)
    assert np.array_equal(np.where(got.codes == sjhip.Context.GROUP_NONE, -1, got.codes.astype(np.int64)), wcodes)
    for (count, not_ok, total, sum_hi, lo, hi), (wcount, wnot, wtotal, wlo, whi) in zip(got.values, aggs):
        assert np.array_equal(count.astype(np.int64), wcount) and np.array_equal(not_ok.astype(np.int64), wnot)
        assert np.array_equal(total, wtotal) and np.array_equal(lo, wlo) and np.array_equal(hi, whi)


def main():
    ctx = sjhip.Context(0)
    names = [a for a in ARGS if a in ("synthetic", "parking")] or ["synthetic", "parking"]
    out_dir = ARGS[ARGS.index("--out") + 1] if "--out" in ARGS else os.path.join(ROOT, "profiles")
    n_rows = int(ARGS[ARGS.index("--rows") + 1]) if "--rows" in ARGS else N
    say(f"# {torch.cuda.get_device_name(0)}; host wall time in ms, median of {REPS} warmed calls, device-resident result, {n_rows} rows")
    for name in names:
        doc, kcols, vcols = document(name, n_rows)
        d, (tl, sl) = resident(ctx, doc)
        k0, v0 = kcols[0], vcols[0]

        full = lambda: ctx.group_paths(kcols, vcols)  # noqa: E731
        build = lambda: ctx.group_paths(kcols, vcols, fetch=False)  # noqa: E731
        table = lambda: ctx.extract_table(kcols + vcols)  # noqa: E731
        host = lambda: host_group(table(), kcols, vcols)  # noqa: E731
        twice = lambda: [ctx.group_path(k0[0], k0[1], path, kind) for path, kind in vcols]  # noqa: E731
        one_multi = lambda: ctx.group_paths([k0], [v0])  # noqa: E731
        one_single = lambda: ctx.group_path(k0[0], k0[1], v0[0], v0[1])  # noqa: E731

        g = full()
        check(g, host())  # results first, times second
        m1, s1 = one_multi(), one_single()
        for x, y in zip([m1.first_row, m1.group_rows, m1.codes, m1.status[0]] + list(m1.values[0]),
                        [s1.first_row, s1.group_rows, s1.codes, s1.status] + list(s1.aggregates())):
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
        assert m1.keys[0] == s1.keys
        runs = {"a": [], "b": [], "c": [], "e": [], "d": [], "m1": [], "s1": []}
        for r in range(SPREAD_RUNS):  # alternating; the expensive host route three times only
            runs["s1"].append(med(one_single))
            runs["m1"].append(med(one_multi))
            runs["a"].append(med(full))
            runs["b"].append(med(build))
            runs["d"].append(med(twice))
            if r < 3:
                runs["c"].append(med(host, reps=3))
                runs["e"].append(med(table, reps=3))
        m = {k: statistics.median(v) for k, v in runs.items()}
        show = lambda k: " ".join("%.3f" % x for x in runs[k])  # noqa: E731
        spread = max(runs["s1"]) - min(runs["s1"])
        diff = m["m1"] - m["s1"]
        what = ", ".join(b".".join(path).decode() for path, _ in kcols)
        vals = ", ".join(b".".join(path).decode() for path, _ in vcols)
        pcie = sum(g.key_bytes) + g.groups * (8 * len(kcols) + 16 + len(kcols) + 48 * len(vcols)) + g.rows * (4 + len(kcols))
        say(f"{name}: {len(doc)} B, tape {tl} words, {g.rows} rows, keys ({what}), values ({vals}), {g.groups} groups, "
            f"{int(g.values[0][0].sum())} OK values in column 0")
        say(f"  spread of group_path([first key], first value), fetched: {SPREAD_RUNS} medians {show('s1')}")
        say(f"      median {m['s1']:.3f} ms, min {min(runs['s1']):.3f}, max {max(runs['s1']):.3f}, spread (max - min) {spread:.3f} ms")
        say(f"  one key: group_paths([first], [first value]), fetched  {m['m1']:10.3f} ms  (medians {show('m1')})")
        say(f"      group_paths - group_path = {diff:+.3f} ms against the spread {spread:.3f} ms: "
            f"{'within the spread (not slower)' if diff <= spread else 'SLOWER than the spread allows'}; ratio {m['m1'] / m['s1']:.3f}")
        say(f"  (a) group_paths(2 keys, 2 values), fetched             {m['a']:10.3f} ms  (medians {show('a')})   PCIe {pcie} B")
        say(f"  (b) group_paths(2 keys, 2 values), not fetched         {m['b']:10.3f} ms  (medians {show('b')})")
        say(f"  (c) extract_table fetched + numpy grouping             {m['c']:10.3f} ms  (medians {show('c')})   (c)/(a) {m['c'] / m['a']:6.2f}")
        say(f"      extract_table fetched, not grouped                 {m['e']:10.3f} ms  (medians {show('e')})")
        say(f"  (d) group_path on the first key, once per value        {m['d']:10.3f} ms  (medians {show('d')})")
        del d
    ctx.close()
    os.makedirs(out_dir, exist_ok=True)
    taken = [int(x.group(1)) for x in (re.match(r"r(\d+)", f) for f in os.listdir(os.path.join(ROOT, "profiles"))) if x]
    path = os.path.join(out_dir, "r%02d_group_multi_time.txt" % (max(taken, default=0) + 1))
    with open(path, "w") as f:
        f.write("\n".join(LINES) + "\n")
    print("written to", path)


if __name__ == "__main__":
    main()
