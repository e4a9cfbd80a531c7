"""Unnest rows on the device-resident tape, next to the calls whose passes it is made of and to the host walk it replaces:
python tools/unnest_time.py [--rows N] [--out DIR]

One document, built here: {"items":[ N parents ]}, every parent {"id":k,"r":<a record of random_nd>,"t":[0 to 7 children]} --
random_nd's records (tests/test_gpu_columns.py) give the tape its mixed texture, the children are numbers, strings and small
objects.  N = 1 M parent rows by default.  Under select_rows(items):
  (a) unnest_rows(t) alone; the selection is put back before every call (select_rows: not timed)
  (b) the same result from the host: the tape fetched (sjhip_fetch) and walked -- FindElement, Array, Advance per parent (tests/unnest_walk.py)
  (c) select_rows(items) on that tape: the tape passes of (a)
  (d) find_path(t) over the parents, fetched: a row-lane pass of the cost of (a)'s
(a) is expected to be at most (c) + (d).  Host wall time of warmed calls; every call ends in a synchronisation.  Median of REPS runs,
three medians each; (b) is run once."""
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = sys.argv[1:]
sys.path[:0] = [os.path.join(ROOT, "simdjson-go_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402  (initialises its HIP runtime first, tests/conftest.py)

import query_walk as Q  # noqa: E402
import rows_walk as RW  # noqa: E402
import sjhip  # noqa: E402
import unnest_walk as UW  # noqa: E402
from test_gpu_columns import random_nd  # noqa: E402

REPS = 15
N = int(ARGS[ARGS.index("--rows") + 1]) if "--rows" in ARGS else 1000000


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


def document(n):
    rnd = random.Random(7)
    recs = random_nd(7, 4096).decode().split("\n")
    kinds = [lambda c: str(c * 37), lambda c: '"tag%d"' % c, lambda c: '{"v":%d}' % c]
    parents = []
    for k in range(n):
        kids = ",".join(kinds[(k + c) % 3](c) for c in range(rnd.randrange(8)))
        parents.append('{"id":%d,"r":%s,"t":[%s]}' % (k, recs[k % len(recs)], kids))
    return ('{"items":[' + ",".join(parents) + "]}").encode()


def main():
    ctx = sjhip.Context(0)
    doc = document(N)
    d = torch.empty(len(doc) + 256, dtype=torch.uint8, device="cuda:0")
    d[:len(doc)].copy_(torch.frombuffer(bytearray(doc), dtype=torch.uint8))
    torch.cuda.synchronize()
    tl, sl = ctx.parse_device(d.data_ptr(), len(doc), ndjson=False, copy_strings=True)
    put_back = lambda: ctx.select_rows((b"items",))  # noqa: E731
    records, parents = put_back()
    _, _, rows = ctx.unnest_rows((b"t",))
    a = [med(lambda: ctx.unnest_rows((b"t",)), setup=put_back) for _ in range(3)]
    ctx.select_records()
    c = [med(put_back) for _ in range(3)]
    put_back()
    dd = [med(lambda: ctx.find_path(b"t")) for _ in range(3)]
    # the host's route, once: fetch the tape, walk it
    t0 = time.perf_counter()
    tape, strings = ctx.fetch(tl, sl)
    t_fetch = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    w = Q.Walk(tape, strings, doc)
    offs, index, sts = RW.select_rows(w, (b"items",))
    want = UW.unnest_rows(RW.RowWalk(w, index), (b"t",), offs, sts)
    t_walk = (time.perf_counter() - t0) * 1e3
    put_back()
    assert ctx.unnest_rows((b"t",)) == (records, parents, rows) and len(want[1]) == rows
    assert np.array_equal(ctx.fetch_rows(records, rows)[1], np.array(want[1], dtype=np.uint64))
    ma, mc, md = statistics.median(a), statistics.median(c), statistics.median(dd)
    lines = [f"# {torch.cuda.get_device_name(0)}; host wall time in ms, median of {REPS} warmed calls, device-resident result",
             f"{len(doc)} B, tape {tl} words, {parents} parent rows, {rows} new rows",
             f"  (a) unnest_rows(t)                         {ma:9.3f} ms  (medians {' '.join('%.3f' % x for x in a)})",
             f"  (b) tape fetched {t_fetch:9.1f} ms + walked on the host {t_walk:9.1f} ms = {t_fetch + t_walk:9.1f} ms   (b)/(a) {(t_fetch + t_walk) / ma:7.0f}",
             f"  (c) select_rows(items)                     {mc:9.3f} ms  (medians {' '.join('%.3f' % x for x in c)})",
             f"  (d) find_path(t) over the parents, fetched {md:9.3f} ms  (medians {' '.join('%.3f' % x for x in dd)})",
             f"  (a) / ((c) + (d))                          {ma / (mc + md):9.2f}"]
    print("\n".join(lines))
    if "--out" in ARGS:
        out_dir = ARGS[ARGS.index("--out") + 1]
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "unnest_time.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
