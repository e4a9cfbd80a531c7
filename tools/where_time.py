"""Row predicates on the device-resident tape, next to the count of the same predicate -- the walk alone:
python tools/where_time.py [parking] [twitter] [--regress] [--pkg DIR]

Two documents of 1 M rows:
  parking   configs[4]: parking-citations x1000 ND, 1 M records, no selection          Make == "HOND"
  twitter   {"statuses":[ twitter.json's 100 statuses x10000 ]} under select_rows      lang == "ja"   (tools/rows_time.py's document)
For each:
  (a) count_where_path(path, EQ_STRING, value)
  (b) where_path of the same predicate; then the selection is put back (select_records / select_rows: not timed)
  (c) where_path, a three-column table over the kept rows with its fetch, the selection put back
  (d) what a caller does today: the same table plus the predicate's column over ALL rows with the fetch, and the mask on the host

--regress: only count_where_path EQ_STRING and EQ_INT on configs[4], REPEATS medians each -- for runs that alternate between two
builds (--pkg DIR: import the package from another tree; it finds its own library).

Host wall time of warmed calls; every call ends in a synchronisation.  Median of REPS runs."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = sys.argv[1:]
PKG = ARGS[ARGS.index("--pkg") + 1] if "--pkg" in ARGS else os.path.join(ROOT, "simdjson-go_amd")
sys.path[:0] = [PKG, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402  (initialises its HIP runtime first, tests/conftest.py)

import fixtures  # noqa: E402
import sjhip  # noqa: E402
import workloads  # noqa: E402

REPS, REPEATS = 15, 5


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


def resident(ctx, doc, nd):
    d = torch.empty(len(doc) + 256, dtype=torch.uint8, device="cuda:0")
    d[:len(doc)].copy_(torch.frombuffer(bytearray(doc), dtype=torch.uint8))
    torch.cuda.synchronize()
    return d, ctx.parse_device(d.data_ptr(), len(doc), ndjson=nd, copy_strings=True)


def host_mask(off, data, value):
    """rows whose string equals `value`: the mask a caller builds from the fetched column"""
    starts, lens = off[:-1].astype(np.int64), np.diff(off.astype(np.int64))
    mask = lens == len(value)
    b = np.frombuffer(data, dtype=np.uint8)
    at = starts[mask]
    eq = np.ones(len(at), dtype=bool)
    for k, ch in enumerate(value):
        eq &= b[at + k] == ch
    mask[np.flatnonzero(mask)[~eq]] = False
    return mask


def regress(ctx):
    doc = workloads.c5_parking_nd(1000).rstrip(b"\n")
    d, (tl, sl) = resident(ctx, doc, True)
    s = [med(lambda: ctx.count_where_path((b"Make",), ctx.OP_EQ_STRING, b"HOND")) for _ in range(REPEATS)]
    i = [med(lambda: ctx.count_where_path((b"Fine amount",), ctx.OP_EQ_INT, 68)) for _ in range(REPEATS)]
    print(f"regress {sjhip._lib.LIB_PATH}: count_where_path on configs[4], ms, {REPEATS} medians of {REPS}")
    print("  EQ_STRING Make HOND     " + " ".join(f"{x:7.4f}" for x in s) + f"   median {statistics.median(s):7.4f} spread {max(s) - min(s):.4f}")
    print("  EQ_INT Fine amount 68   " + " ".join(f"{x:7.4f}" for x in i) + f"   median {statistics.median(i):7.4f} spread {max(i) - min(i):.4f}")


def main():
    ctx = sjhip.Context(0)
    if "--regress" in ARGS:
        return regress(ctx)
    names = [a for a in ARGS if a in ("parking", "twitter")] or ["parking", "twitter"]
    print(f"# {torch.cuda.get_device_name(0)}; host wall time in ms, median of {REPS} warmed calls, device-resident result")
    for name in names:
        if name == "parking":
            doc, nd, base = workloads.c5_parking_nd(1000).rstrip(b"\n"), True, None
            path, value = (b"Make",), b"HOND"
            columns = [((b"Fine amount",), ctx.COL_STRING_CVT), ((b"Latitude",), ctx.COL_STRING_CVT), ((b"Color",), ctx.COL_STRING)]
        else:
            statuses = json.loads(fixtures.load("twitter"))["statuses"]
            one = ",".join(json.dumps(s, separators=(",", ":"), ensure_ascii=False) for s in statuses)
            doc, nd, base = ('{"statuses":[' + ",".join([one] * 10000) + "]}").encode(), False, (b"statuses",)
            path, value = (b"lang",), b"ja"
            columns = [((b"id",), ctx.COL_INT), ((b"user", b"screen_name"), ctx.COL_STRING), ((b"retweet_count",), ctx.COL_FLOAT)]
        d, (tl, sl) = resident(ctx, doc, nd)
        put_back = ctx.select_records if base is None else (lambda: ctx.select_rows(base))
        put_back()
        rows_all = ctx.count_where_path(path, ctx.OP_EXISTS)
        a = [med(lambda: ctx.count_where_path(path, ctx.OP_EQ_STRING, value)) for _ in range(3)]
        b = [med(lambda: ctx.where_path(path, ctx.OP_EQ_STRING, value), setup=put_back) for _ in range(3)]
        put_back()
        records, kept = ctx.where_path(path, ctx.OP_EQ_STRING, value)
        assert kept == ctx.count_where_path(path, ctx.OP_EXISTS)

        def filtered_table():
            ctx.where_path(path, ctx.OP_EQ_STRING, value)
            return ctx.extract_table(columns)

        def masked_table():
            table = ctx.extract_table(columns + [(path, ctx.COL_STRING)])
            mask = host_mask(table[-1][0], table[-1][1], value)
            out = []
            for col in table[:-1]:
                if len(col) == 2:
                    out.append((col[0][mask], col[1][mask]))
                else:  # a string column: the kept lengths; the bytes would be gathered from them
                    out.append((np.diff(col[0].astype(np.int64))[mask], col[2][mask]))
            return int(mask.sum())

        put_back()
        assert masked_table() == kept
        c = med(filtered_table, setup=put_back, reps=7)
        put_back()
        dd = med(masked_table, reps=7)
        ma, mb = statistics.median(a), statistics.median(b)
        print(f"{name}: {len(doc)} B, tape {tl} words, {records} records, {rows_all} rows, {kept} kept by {path[0].decode()} == {value.decode()}")
        print(f"  (a) count_where_path EQ_STRING   {ma:8.3f} ms  (medians {' '.join('%.3f' % x for x in a)})")
        print(f"  (b) where_path                   {mb:8.3f} ms  (medians {' '.join('%.3f' % x for x in b)})   (b)/(a) {mb / ma:5.2f}")
        print(f"  (c) where_path + table of 3 columns over the kept rows, fetched   {c:9.3f} ms")
        print(f"  (d) table of 3 + 1 columns over all rows, fetched, host mask       {dd:9.3f} ms   (d)/(c) {dd / c:5.2f}")
        ctx.select_records()
        del d
    ctx.close()


if __name__ == "__main__":
    main()
