"""Aggregates on the device-resident tape, next to the column they reduce and to the count of the same walk:
python tools/aggregate_time.py [parking] [twitter]

Two documents of 1 M rows:
  parking   configs[4]: parking-citations x1000 ND, 1 M records, no selection      path Fine     (every member of this document is
            a string -- "Fine":"50" --, so the conversion refuses every row: the walk and the reduction run, nothing is summed)
  twitter   {"statuses":[ twitter.json's 100 statuses x10000 ]} under select_rows   path retweet_count, INT   (tools/rows_time.py's
            document: one record owns every row)
For each, alternating on the same device:
  (a) count_where_path(path, EXISTS)                              the walk alone, 8 bytes back
  (b) aggregate_path(path, kind)                                  88 bytes back
  (c) aggregate_path_records(path, kind)                          six arrays of one entry per record back
  (d) extract_path(path, kind) and the reduction with numpy       9 bytes per row back: what a caller does today

Host wall time of warmed calls; every call ends in a synchronisation.  Median of REPS runs, three medians each."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = sys.argv[1:]
sys.path[:0] = [os.path.join(ROOT, "simdjson-go_amd"), os.path.join(ROOT, "tests")]
import torch  # noqa: E402  (initialises its HIP runtime first, tests/conftest.py)

import fixtures  # noqa: E402
import sjhip  # noqa: E402
import workloads  # noqa: E402

REPS = 15


def med(fn, reps=REPS):
    """median wall time of fn() in ms"""
    ts = []
    for k in range(reps + 2):
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


def main():
    ctx = sjhip.Context(0)
    names = [a for a in ARGS if a in ("parking", "twitter")] or ["parking", "twitter"]
    print(f"# {torch.cuda.get_device_name(0)}; host wall time in ms, median of {REPS} warmed calls, device-resident result")
    for name in names:
        if name == "parking":
            doc, nd, base = workloads.c5_parking_nd(1000).rstrip(b"\n"), True, None
            path, kind = (b"Fine",), ctx.COL_FLOAT
        else:
            statuses = json.loads(fixtures.load("twitter"))["statuses"]
            one = ",".join(json.dumps(s, separators=(",", ":"), ensure_ascii=False) for s in statuses)
            doc, nd, base = ('{"statuses":[' + ",".join([one] * 10000) + "]}").encode(), False, (b"statuses",)
            path, kind = (b"retweet_count",), ctx.COL_INT
        d, (tl, sl) = resident(ctx, doc, nd)
        if base is not None:
            ctx.select_rows(base)

        def host_reduce():
            vals, st = ctx.extract_path(path, kind)
            ok = vals[st == ctx.COL_OK]
            if len(ok) == 0:
                return len(vals), 0, 0, None, None
            total = float(ok.sum()) if kind == ctx.COL_FLOAT else int(ok.sum())
            return len(vals), len(ok), total, ok.min(), ok.max()

        agg, per, host = ctx.aggregate_path(path, kind), ctx.aggregate_path_records(path, kind), host_reduce()
        assert (agg.rows, agg.count) == host[:2] and (agg.count == 0 or (agg.sum, agg.min, agg.max) == host[2:]), (agg, host)
        assert int(per[0].sum()) == agg.count and int(per[0].sum() + per[1].sum()) == agg.rows
        runs = {"a": [], "b": [], "c": [], "d": [], "e": []}
        for _ in range(3):  # alternating
            runs["a"].append(med(lambda: ctx.count_where_path(path, ctx.OP_EXISTS)))
            runs["b"].append(med(lambda: ctx.aggregate_path(path, kind)))
            runs["c"].append(med(lambda: ctx.aggregate_path_records(path, kind)))
            runs["d"].append(med(host_reduce, reps=7))
            runs["e"].append(med(lambda: ctx.extract_path(path, kind), reps=7))
        m = {k: statistics.median(v) for k, v in runs.items()}
        show = lambda k: " ".join("%.3f" % x for x in runs[k])  # noqa: E731
        print(f"{name}: {len(doc)} B, tape {tl} words, {len(per[0])} records, {agg.rows} rows, path {path[0].decode()} kind {kind}: {agg}")
        print(f"  (a) count_where_path EXISTS                   {m['a']:9.3f} ms  (medians {show('a')})")
        print(f"  (b) aggregate_path                            {m['b']:9.3f} ms  (medians {show('b')})   (b)/(a) {m['b'] / m['a']:5.2f}")
        print(f"  (c) aggregate_path_records                    {m['c']:9.3f} ms  (medians {show('c')})")
        print(f"  (d) extract_path + numpy reduction            {m['d']:9.3f} ms  (medians {show('d')})   (d)/(b) {m['d'] / m['b']:5.2f}")
        print(f"      extract_path alone                        {m['e']:9.3f} ms  (medians {show('e')})   /(b)    {m['e'] / m['b']:5.2f}")
        ctx.select_records()
        del d
    ctx.close()


if __name__ == "__main__":
    main()
