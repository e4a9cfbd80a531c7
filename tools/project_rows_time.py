"""The selected rows projected onto three paths as NDJSON text, next to the rows written back whole and to a table formatted on
the host:
python tools/project_rows_time.py [--trace]

configs[4]: parking-citations x1000 ND, 1 M records resident on the device, parsed with SJHIP_FLAG_KEY_FLAGS.  Two selections:
  kept   where_path(("Make",), EQ_STRING, "HOND")     -- 116 000 rows
  all    where_path((), EXISTS)                       -- every record a row
and on each, the text staying on the device and every call ending in a device synchronisation:
  (p) marshal_rows_paths of Ticket, Make, Fine                              -- the projection
  (a) marshal_rows of the same selection                                    -- the yardstick: the same rows written back whole
  (b) extract_table of the same three paths as string columns, fetched, and formatted as the same NDJSON lines on the host
  (c) the bytes each of them moves over PCIe: (p) and (a) with their fetch (text and offsets), (b)'s columns
The selecting call itself is set up before every timed call and not timed.

Host wall time of warmed calls: REPEATS medians of REPS runs each, their median and their spread (max - min).  --trace: 10 x [(p);
(a)] on both selections and nothing else -- for a run under rocprofv3 --kernel-trace --stats."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = sys.argv[1:]
sys.path[:0] = [os.path.join(ROOT, "simdjson-go_amd"), os.path.join(ROOT, "tests")]
import torch  # noqa: E402  (initialises its HIP runtime first, tests/conftest.py)

import sjhip  # noqa: E402
import workloads  # noqa: E402

REPS, REPEATS = 15, 5
FIELDS = (b"Ticket", b"Make", b"Fine")
COLUMNS = [(f,) for f in FIELDS]


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
    return f"  {label:<58s} {statistics.median(xs):8.3f} ms   spread {max(xs) - min(xs):.3f}   (medians {' '.join('%.3f' % x for x in xs)})"


def host_lines(cols):
    """the table's three string columns as the NDJSON lines the projection writes (json.dumps escapes what escapeBytes escapes on
    these fields: they are plain ASCII)"""
    parts = []
    for f, (off, data, status) in zip(FIELDS, cols):
        o = off.tolist()
        name = json.dumps(f.decode())
        parts.append([name + ':"' + data[o[i]:o[i + 1]].decode() + '"' if status[i] == 0 else None for i in range(len(o) - 1)])
    return "\n".join("{" + ",".join(x for x in row if x is not None) + "}" for row in zip(*parts)).encode()


def main():
    ctx = sjhip.Context(0)
    doc = workloads.c5_parking_nd(1000).rstrip(b"\n")
    d = torch.empty(len(doc) + 256, dtype=torch.uint8, device="cuda:0")
    d[:len(doc)].copy_(torch.frombuffer(bytearray(doc), dtype=torch.uint8))
    torch.cuda.synchronize()
    tl, sl = ctx.parse_device(d.data_ptr(), len(doc), ndjson=True, copy_strings=True, key_flags=True)
    S = ctx.COL_STRING

    selections = {
        "kept": lambda: (ctx.select_records(), ctx.where_path((b"Make",), ctx.OP_EQ_STRING, b"HOND")),
        "all": lambda: (ctx.select_records(), ctx.where_path((), ctx.OP_EXISTS)),
    }

    def p(fetch=False):
        return ctx.marshal_rows_paths(COLUMNS, fetch=fetch, offsets=fetch)

    def a(fetch=False):
        return ctx.marshal_rows(fetch=fetch, offsets=fetch)

    def b_device():
        return ctx.extract_table([(c, S) for c in COLUMNS], fetch=False)

    def b():
        return host_lines(ctx.extract_table([(c, S) for c in COLUMNS]))

    if "--trace" in ARGS:
        for _ in range(10):
            for select in selections.values():
                select()
                p()
                a()
        torch.cuda.synchronize()
        return ctx.close()
    print(f"# {torch.cuda.get_device_name(0)}; {sjhip._lib.LIB_PATH}")
    print(f"# configs[4]: {len(doc)} B, tape {tl} words, Strings.B {sl} B; columns {', '.join(f.decode() for f in FIELDS)}")
    print(f"# host wall time, ms, {REPEATS} medians of {REPS} warmed calls; the selecting call is not timed")
    for what, select in selections.items():
        select()
        n, text, off = p(True)
        n_a, whole, off_a = a(True)
        cols = ctx.extract_table([(c, S) for c in COLUMNS])
        assert n == n_a and host_lines(cols) == text  # the three ways agree
        moved_b = sum(o.nbytes + len(dat) + st.nbytes for o, dat, st in cols)
        print(f"{what}: {n} rows; projected text {len(text)} B, whole rows {len(whole)} B")
        xp = [med(p, setup=select) for _ in range(REPEATS)]
        xa = [med(a, setup=select) for _ in range(REPEATS)]
        xt = [med(b_device, setup=select) for _ in range(REPEATS)]
        print(line("(p) marshal_rows_paths, 3 of the fields", xp))
        print(line("(a) marshal_rows, the rows whole", xa))
        print(line("    extract_table, 3 string columns, on the device", xt))
        print(f"  (p) / (a) = {statistics.median(xp) / statistics.median(xa):.2f} for {len(text) / len(whole):.2f} of the text")
        xpf = [med(lambda: p(True), setup=select, reps=5) for _ in range(3)]
        xaf = [med(lambda: a(True), setup=select, reps=5) for _ in range(3)]
        xbf = [med(b, setup=select, reps=1) for _ in range(2)]  # (seconds each: the host formats every row)
        print(line("(p) + fetch of text and offsets", xpf))
        print(line("(a) + fetch of text and offsets", xaf))
        print(line("(b) extract_table + fetch + the lines formatted on the host", xbf))
        print(f"  (c) bytes over PCIe: (p) {len(text) + off.nbytes}, (a) {len(whole) + off_a.nbytes}, (b) {moved_b}")
    ctx.close()


if __name__ == "__main__":
    main()
