"""The selected rows as NDJSON text, next to MarshalJSON of the whole result:
python tools/marshal_rows_time.py [--trace] [--pkg DIR]

configs[4]: parking-citations x1000 ND, 1 M records resident on the device, parsed with SJHIP_FLAG_KEY_FLAGS:
  (a) marshal_json of the whole result                                     -- the yardstick (k_ms_tile: the parent commit's code)
  (b) where_path(("Make",), EQ_STRING, "HOND") followed by marshal_rows    -- 116 000 rows; select_records first, not timed
  (c) where_path((), EXISTS) followed by marshal_rows                      -- every record a row: the same text as (a)
  (d) (b) followed by the fetch of text and offsets, (a) followed by the fetch of its text

Host wall time of warmed calls; in (a) - (c) the text stays on the device and every call ends in a device synchronisation.
REPEATS medians of REPS runs each, their median and their spread (max - min).  --trace: 10 x [(a); (b); (c)] and nothing else --
for a run under rocprofv3 --kernel-trace --stats.  --pkg DIR: import the package from another tree (it finds its own library); a
tree without marshal_rows times (a) and its fetch alone."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = sys.argv[1:]
PKG = ARGS[ARGS.index("--pkg") + 1] if "--pkg" in ARGS else os.path.join(ROOT, "simdjson-go_amd")
sys.path[:0] = [PKG, os.path.join(ROOT, "tests")]
import torch  # noqa: E402  (initialises its HIP runtime first, tests/conftest.py)

import sjhip  # noqa: E402
import workloads  # noqa: E402

REPS, REPEATS = 15, 5


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
    return f"  {label:<52s} {statistics.median(xs):8.3f} ms   spread {max(xs) - min(xs):.3f}   (medians {' '.join('%.3f' % x for x in xs)})"


def main():
    ctx = sjhip.Context(0)
    doc = workloads.c5_parking_nd(1000).rstrip(b"\n")
    d = torch.empty(len(doc) + 256, dtype=torch.uint8, device="cuda:0")
    d[:len(doc)].copy_(torch.frombuffer(bytearray(doc), dtype=torch.uint8))
    torch.cuda.synchronize()
    tl, sl = ctx.parse_device(d.data_ptr(), len(doc), ndjson=True, copy_strings=True, key_flags=True)
    have = hasattr(ctx, "marshal_rows")

    def a(fetch=False):
        return ctx.marshal_json(fetch=fetch)

    def b(fetch=False):
        ctx.where_path((b"Make",), ctx.OP_EQ_STRING, b"HOND")
        return ctx.marshal_rows(fetch=fetch, offsets=fetch)

    def c():
        ctx.where_path((), ctx.OP_EXISTS)
        return ctx.marshal_rows(fetch=False)

    whole = a(True)
    kept = (0, 0)
    if have:  # (c) delivers the text of (a); (b) the lines of it that hold the make
        ctx.where_path((), ctx.OP_EXISTS)
        n, text = ctx.marshal_rows()
        assert text == whole and n == text.count(b"\n") + 1
        ctx.select_records()
        n, text, off = b(True)
        assert text == b"\n".join(l for l in whole.split(b"\n") if b'"Make":"HOND"' in l) and n == len(off) - 1
        kept = (n, len(text))
        ctx.select_records()
    if "--trace" in ARGS:
        for _ in range(10):
            a()
            if have:
                b()
                ctx.select_records()
                c()
                ctx.select_records()
        torch.cuda.synchronize()
        return ctx.close()
    print(f"# {torch.cuda.get_device_name(0)}; {sjhip._lib.LIB_PATH}")
    print(f"# configs[4]: {len(doc)} B, tape {tl} words, Strings.B {sl} B; text {len(whole)} B; Make == HOND: {kept[0]} rows, {kept[1]} B")
    print(f"# host wall time, ms, {REPEATS} medians of {REPS} warmed calls")
    xa = [med(a) for _ in range(REPEATS)]
    print(line("(a) marshal_json, the whole result", xa))
    if have:
        xb = [med(b, setup=ctx.select_records) for _ in range(REPEATS)]
        xc = [med(c, setup=ctx.select_records) for _ in range(REPEATS)]
        ctx.select_records()
        print(line("(b) where_path EQ_STRING + marshal_rows", xb))
        print(line("(c) where_path EXISTS + marshal_rows (all rows)", xc))
        print(f"  (c) / (a) = {statistics.median(xc) / statistics.median(xa):.2f}; (b) / (c) = {statistics.median(xb) / statistics.median(xc):.2f} "
              f"for {kept[1] / len(whole):.2f} of the text")
    xaf = [med(lambda: a(True), reps=5) for _ in range(3)]
    print(line("(d) marshal_json + fetch", xaf))
    if have:
        xbf = [med(lambda: b(True), setup=ctx.select_records, reps=5) for _ in range(3)]
        print(line("(d) where_path EQ_STRING + marshal_rows + fetch", xbf))
    ctx.close()


if __name__ == "__main__":
    main()
