"""Tables against the single-column calls on configs[4] (parking-citations x1000 ND, 1 M records, device-resident):
python tools/table_time.py

For k = 1, 2, 4, 8 top-level parking keys, once with every column STRING_CVT and once with numeric kinds mixed in:
  (a) the sum of the k existing single-column calls (extract_path / extract_path_strings, fetch=False) -- kernels the tables leave
      untouched --, measured REPEATS times: the spread of its medians is the yardstick
  (b) extract_table of the same columns (fetch=False)
  (c) both including the fetches: host -> host

Host wall time of warmed calls; every call ends in a synchronisation.  Median of REPS runs."""
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

REPS, REPEATS = 15, 3
KEYS = [b"Make", b"Latitude", b"Color", b"Fine", b"Ticket", b"Agency", b"RPState", b"Longitude"]  # (Make is the 9th member, Longitude the last)


def med(fn, reps=REPS):
    fn()
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1e3


def main():
    doc = workloads.c5_parking_nd(1000).rstrip(b"\n")
    ctx = sjhip.Context(0)
    d = torch.empty(len(doc) + 256, dtype=torch.uint8, device="cuda:0")
    d[:len(doc)].copy_(torch.frombuffer(bytearray(doc), dtype=torch.uint8))
    torch.cuda.synchronize()
    tl, sl = ctx.parse_device(d.data_ptr(), len(doc), ndjson=True, copy_strings=True)
    print(f"# configs[4]: parking-citations x1000 ND, {len(doc)} B, tape {tl} words, Strings.B {sl} B, device-resident, "
          f"{torch.cuda.get_device_name(0)}; host wall time in ms, median of {REPS} warmed calls; (a) measured {REPEATS} times")
    S, SC = ctx.COL_STRING, ctx.COL_STRING_CVT
    mixes = {"all STRING_CVT": [SC] * 8, "mixed": [SC, ctx.COL_FLOAT, S, ctx.COL_INT, ctx.COL_UINT, SC, S, ctx.COL_FLOAT]}

    def single(path, kind, fetch):
        if kind in (S, SC):
            return ctx.extract_path_strings(path, cvt=kind == SC, fetch=fetch)
        return ctx.extract_path(path, kind)  # (the numeric call always brings its 9 bytes per record back)

    for name, kinds in mixes.items():
        print(f"{name}")
        for k in (1, 2, 4, 8):
            columns = [((key,), kind) for key, kind in zip(KEYS[:k], kinds)]
            table = ctx.extract_table(columns)
            for (path, kind), col in zip(columns, table):  # the same columns
                want = single(path, kind, True)
                assert all(np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(col, want)), (path, kind)
            a = [med(lambda: [single(p, kd, False) for p, kd in columns]) for _ in range(REPEATS)]
            b = med(lambda: ctx.extract_table(columns, fetch=False))
            a_f = [med(lambda: [single(p, kd, True) for p, kd in columns], reps=7) for _ in range(REPEATS)]
            b_f = med(lambda: ctx.extract_table(columns), reps=7)
            spread, spread_f = max(a) - min(a), max(a_f) - min(a_f)
            print(f"  k={k}  (a) single calls {statistics.median(a):8.3f} (spread {spread:.3f})   (b) extract_table {b:8.3f}   "
                  f"(a)-(b) {statistics.median(a) - b:+8.3f}   {statistics.median(a) / b:5.2f}x")
            print(f"       (c) with fetches: single {statistics.median(a_f):8.3f} (spread {spread_f:.3f})   table {b_f:8.3f}   "
                  f"{statistics.median(a_f) / b_f:5.2f}x")
    ctx.close()


if __name__ == "__main__":
    main()
