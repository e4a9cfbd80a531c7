"""The row selection on the device-resident tape, next to the serializer -- the only other whole-tape pass with scans:
python tools/rows_time.py

Two documents, one record each, >= 1 M rows:
  twitter   {"statuses":[ twitter.json's 100 statuses, repeated to >= 1 M ]}                    select_rows(statuses)
  parking   configs[4]'s records (parking-citations x1000, 1 M lines) as one root array [...]    select_rows() -- the empty path
For each:
  (a) select_rows                                 (b) serialize (fetch=False) on the same tape
  (c) a three-column table over the rows (fetch=False), in all and per row -- tools/table_time.py has the per-record figure of
      the same walk over NDJSON records
  (d) a host walk of the fetched tape: fetch + Array.Iter / Advance over the elements in Python (the first 100 000 rows, scaled)

Host wall time of warmed calls; every call ends in a synchronisation.  Median of REPS runs."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "simdjson-go_amd"), os.path.join(ROOT, "tests")]
import torch  # noqa: E402  (initialises its HIP runtime first, tests/conftest.py)

import fixtures  # noqa: E402
import sjhip  # noqa: E402
import workloads  # noqa: E402

REPS = 15
MASK = 0x00FFFFFFFFFFFFFF


def med(fn, reps=REPS):
    fn()
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1e3


def host_walk(tape, first, limit):
    """Array.Iter / Advance from the '[' at `first`: the tape index of up to `limit` elements; -> (elements, seconds)"""
    t0 = time.perf_counter()
    i, end, n = first + 1, (int(tape[first]) & MASK) - 1, 0
    while i < end and n < limit:
        w = int(tape[i])
        tag = chr(w >> 56)
        i = (w & MASK) if tag in "{[" else i + 2 if tag in '"lud' else i + 1
        n += 1
    return n, time.perf_counter() - t0


def main():
    statuses = json.loads(fixtures.load("twitter"))["statuses"]
    one = ",".join(json.dumps(s, separators=(",", ":"), ensure_ascii=False) for s in statuses)
    twitter = ('{"statuses":[' + ",".join([one] * 10000) + "]}").encode()
    parking = b"[" + workloads.c5_parking_nd(1000).rstrip(b"\n").replace(b"\n", b",") + b"]"
    docs = [("twitter statuses x10000", twitter, (b"statuses",), [((b"id",), 1), ((b"user", b"screen_name"), 4), ((b"retweet_count",), 0)]),
            ("parking x1000 as a root array", parking, (), [((b"Make",), 5), ((b"Fine",), 1), ((b"Latitude",), 0)])]
    ctx = sjhip.Context(0)
    print(f"# {torch.cuda.get_device_name(0)}; host wall time in ms, median of {REPS} warmed calls, device-resident result")
    for name, doc, path, columns in docs:
        d = torch.empty(len(doc) + 256, dtype=torch.uint8, device="cuda:0")
        d[:len(doc)].copy_(torch.frombuffer(bytearray(doc), dtype=torch.uint8))
        torch.cuda.synchronize()
        tl, sl = ctx.parse_device(d.data_ptr(), len(doc), ndjson=False, copy_strings=True)
        ctx.select_records()
        t_ser = med(lambda: ctx.serialize(fetch=False))
        t_sel = med(lambda: ctx.select_rows(path))
        records, rows = ctx.select_rows(path)
        t_tab = med(lambda: ctx.extract_table(columns, fetch=False))
        t0 = time.perf_counter()
        tape, _ = ctx.fetch(tl, sl)
        t_fetch = time.perf_counter() - t0
        off, idx, st = ctx.fetch_rows(records, rows)
        n, t_walk = host_walk(tape, int(idx[0]) - 1 if path == () else int(ctx_find(ctx, path)), 100000)
        print(f"{name}: {len(doc)} B, tape {tl} words, {records} record, {rows} rows")
        print(f"  (a) select_rows {t_sel:9.3f} ms   (b) serialize {t_ser:9.3f} ms   (a)/(b) {t_sel / t_ser:5.2f}")
        print(f"  (c) table of 3 columns over the rows {t_tab:9.3f} ms = {t_tab * 1e6 / rows:7.1f} ns per row")
        print(f"  (d) host: fetch {t_fetch * 1e3:9.1f} ms + walk {t_walk * 1e3 * rows / n:9.1f} ms ({n} elements walked, scaled to {rows})")
        del d


def ctx_find(ctx, path):
    ctx.select_records()
    v = ctx.find_path(*path)[0]
    ctx.select_rows(path)
    return v


if __name__ == "__main__":
    main()
