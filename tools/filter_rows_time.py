"""The selected rows as a (Tape, Strings.B), next to the filter that predates the row selection:
python tools/filter_rows_time.py [--fetch] [--trace] [--pkg DIR]

configs[4]: parking-citations x1000 ND, 1 M records resident on the device, Make == "HOND" (348 000 records):
  (a) filter_where("Make", "HOND")                                         -- the yardstick (its code is the parent commit's)
  (b) where_path(("Make",), EQ_STRING, "HOND") followed by filter_rows     -- the selection put back first (select_records: not timed)
  (c) filter_rows alone, on the selection (b) leaves

Host wall time of warmed calls; the result stays on the device and every call ends in a device synchronisation (--fetch: the
result is fetched instead, which adds its D2H copy to all three).  REPEATS medians of REPS runs each, their median and their
spread (max - min).  --trace: 10 x [(a); select_records; (b); (c)] and nothing else -- for a run under rocprofv3 --kernel-trace --stats.
--pkg DIR: import the package from another tree (it finds its own library); a tree without filter_rows times (a) alone."""
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

import sjhip  # noqa: E402
import workloads  # noqa: E402

REPS, REPEATS = 15, 5
FETCH = "--fetch" in ARGS


def med(fn, setup=None, reps=REPS):
    """median wall time of fn() in ms; setup() runs before every call and is not timed"""
    ts = []
    for k in range(reps + 2):
        if setup:
            setup()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if k >= 2:
            ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1e3


def line(label, xs):
    return f"  {label:<44s} {statistics.median(xs):8.3f} ms   spread {max(xs) - min(xs):.3f}   (medians {' '.join('%.3f' % x for x in xs)})"


def main():
    ctx = sjhip.Context(0)
    doc = workloads.c5_parking_nd(1000).rstrip(b"\n")
    d = torch.empty(len(doc) + 256, dtype=torch.uint8, device="cuda:0")
    d[:len(doc)].copy_(torch.frombuffer(bytearray(doc), dtype=torch.uint8))
    torch.cuda.synchronize()
    tl, sl = ctx.parse_device(d.data_ptr(), len(doc), ndjson=True, copy_strings=True)
    have = hasattr(ctx, "filter_rows")

    def a():
        return ctx.filter_where(b"Make", b"HOND", fetch=FETCH)

    def b():
        ctx.where_path((b"Make",), ctx.OP_EQ_STRING, b"HOND")
        return ctx.filter_rows(fetch=FETCH)

    def c():
        return ctx.filter_rows(fetch=FETCH)

    n, sub = ctx.filter_where(b"Make", b"HOND")
    if have:  # the three deliver the same bytes
        ctx.where_path((b"Make",), ctx.OP_EQ_STRING, b"HOND")
        n2, skipped, pj = ctx.filter_rows()
        assert (n2, skipped) == (n, 0) and np.array_equal(pj.Tape, sub.Tape) and np.array_equal(pj.Strings, sub.Strings)
        ctx.select_records()
    if "--trace" in ARGS:
        for _ in range(10):
            a()
            if have:
                ctx.select_records()
                b()
                c()
        torch.cuda.synchronize()
        return ctx.close()
    print(f"# {torch.cuda.get_device_name(0)}; {sjhip._lib.LIB_PATH}")
    print(f"# configs[4]: {len(doc)} B, tape {tl} words, Strings.B {sl} B, {n} of 1 M records kept: result {len(sub.Tape)} words, {len(sub.Strings)} B")
    print(f"# host wall time, ms, {REPEATS} medians of {REPS} warmed calls; the result {'fetched' if FETCH else 'left on the device'}")
    xa = [med(a) for _ in range(REPEATS)]
    print(line('(a) filter_where("Make", "HOND")', xa))
    if have:
        xb = [med(b, setup=ctx.select_records) for _ in range(REPEATS)]
        ctx.select_records()
        ctx.where_path((b"Make",), ctx.OP_EQ_STRING, b"HOND")
        xc = [med(c) for _ in range(REPEATS)]
        print(line("(b) where_path EQ_STRING + filter_rows", xb))
        print(line("(c) filter_rows alone", xc))
        ma, mc = statistics.median(xa), statistics.median(xc)
        print(f"  (c) - (a) = {mc - ma:+.3f} ms; the spread of (a) is {max(xa) - min(xa):.3f} ms")
    ctx.close()


if __name__ == "__main__":
    main()
