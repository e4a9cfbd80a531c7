"""Order rows on the device-resident tape, next to the host route a caller had before:
python tools/order_time.py [parking] [digits3] [digits8] [missing10] [--out DIR]

Four documents of 1 M rows, ND, no selection (the rows are the records):
  parking   configs[4]: parking-citations x1000 ND, key Fine FLOAT.  Every member of this document is a string, so no key converts:
            the walk, the compaction and the narrowing run, the sort takes no pass
  digits3   {"id":<r>,"retweet_count":<below 2^20>,"text":"..."}: three digits of the key vary, the plan takes three passes
  digits8   the same rows with a random 64-bit key under INT: all eight digits vary
  missing10 the rows of digits3, one in ten without the key member: the rows without a key travel through both sorts
For each, alternating on the same device:
  (a) order_path(key, kind, descending, limit=10) + marshal_rows, fetched     "the 10 largest", as text, and nothing else over PCIe
  (b) order_path(key, kind, limit=0), fetched                                 the full ORDER BY: order, values, status of every row
  (c) extract_path(key, kind), fetched, + numpy.argsort(kind="stable")       the route of the parent commit (which has no way back
      to the device with the row numbers it found)
Host wall time of warmed calls; every call ends in a synchronisation.  Median of REPS runs, three medians each.  The pass count is
the plan of csrc/sj_sort.h on the keys of the column (tests/order_walk.pass_mask).  The output is also written to
DIR/rNN_order_time.txt (DIR: profiles/ of the repository), NN the next free number."""
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

REPS = 9
N = 1000000
LINES = []


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


def document(ctx, name):
    if name == "parking":
        return workloads.c5_parking_nd(1000).rstrip(b"\n"), (b"Fine",), ctx.COL_FLOAT
    rnd = random.Random(6)
    if name in ("digits3", "missing10"):
        key = lambda: rnd.randrange(1 << 20)  # noqa: E731
    else:
        key = lambda: rnd.randrange(-(1 << 63), 1 << 63)  # noqa: E731
    lines = ['{"id":%d,"retweet_count":%d,"text":"status number %d"}' % (r, key(), r) for r in range(N)]
    if name == "missing10":
        lines = ['{"id":%d,"text":"status number %d"}' % (r, r) if r % 10 == 9 else line for r, line in enumerate(lines)]
    return "\n".join(lines).encode(), (b"retweet_count",), ctx.COL_INT


def pass_count(vals, st, kind):
    ok = st == 0
    if int(ok.sum()) < 2:
        return 0
    keys = vals[ok].view(np.uint64).copy()
    if kind == 1:
        keys ^= np.uint64(1 << 63)
    elif kind == 0:
        neg = (keys >> np.uint64(63)).astype(bool)
        keys = np.where(neg, ~keys, keys ^ np.uint64(1 << 63))
    varying = int(np.bitwise_and.reduce(keys)) ^ int(np.bitwise_or.reduce(keys))
    return sum(1 for p in range(8) if (varying >> (8 * p)) & 0xFF)


def main():
    ctx = sjhip.Context(0)
    names = [a for a in ARGS if a in ("parking", "digits3", "digits8", "missing10")] or ["parking", "digits3", "digits8", "missing10"]
    out_dir = ARGS[ARGS.index("--out") + 1] if "--out" in ARGS else os.path.join(ROOT, "profiles")
    say(f"# {torch.cuda.get_device_name(0)}; host wall time in ms, median of {REPS} warmed calls, device-resident result, 1 M rows")
    for name in names:
        doc, key, kind = document(ctx, name)
        d, (tl, sl) = resident(ctx, doc)

        def top10():
            ctx.select_records()
            o = ctx.order_path(key, kind, descending=True, limit=10)
            return o, ctx.marshal_rows(offsets=True)

        def full():
            ctx.select_records()
            return ctx.order_path(key, kind)

        def full_device_only():
            ctx.select_records()
            return ctx.order_path(key, kind, fetch=False)

        def host():
            vals, st = ctx.extract_path(key, kind)
            ok = np.flatnonzero(st == ctx.COL_OK)
            return vals, st, np.concatenate([ok[np.argsort(vals[ok], kind="stable")], np.flatnonzero(st != ctx.COL_OK)])

        o = full()
        vals, st, perm = host()
        assert o.rows == len(vals) and np.array_equal(o.order.astype(np.int64), perm)  # (ascending: -0.0 and 0.0 do not meet here)
        top, (n10, text, off) = top10()
        assert top.rows == 10 == n10
        passes = pass_count(vals, st, kind)
        runs = {"a": [], "b": [], "n": [], "c": [], "e": []}
        for _ in range(3):  # alternating
            runs["a"].append(med(top10))
            runs["b"].append(med(full))
            runs["n"].append(med(full_device_only))
            runs["c"].append(med(host, reps=3))
            runs["e"].append(med(lambda: ctx.extract_path(key, kind), reps=3))
        ctx.select_records()
        m = {k: statistics.median(v) for k, v in runs.items()}
        show = lambda k: " ".join("%.3f" % x for x in runs[k])  # noqa: E731
        n = len(vals)
        say(f"{name}: {len(doc)} B, tape {tl} words, {n} rows, {int((st == 0).sum())} with an OK key, key {key[-1].decode()} kind {kind}, {passes} sort passes")
        say(f"  (a) order_path(limit=10, descending) + marshal_rows  {m['a']:10.3f} ms  (medians {show('a')})   PCIe {170 + len(text) + 88} B")
        say(f"  (b) order_path(limit=0), fetched                     {m['b']:10.3f} ms  (medians {show('b')})   PCIe {17 * n} B")
        say(f"      order_path(limit=0), not fetched                 {m['n']:10.3f} ms  (medians {show('n')})")
        say(f"  (c) extract_path fetched + numpy stable argsort      {m['c']:10.3f} ms  (medians {show('c')})   (c)/(a) {m['c'] / m['a']:6.2f}  (c)/(b) {m['c'] / m['b']:6.2f}   PCIe {9 * n} B")
        say(f"      extract_path fetched, not sorted                 {m['e']:10.3f} ms  (medians {show('e')})")
        del d
    ctx.close()
    os.makedirs(out_dir, exist_ok=True)
    taken = [int(x.group(1)) for x in (re.match(r"r(\d+)", f) for f in os.listdir(out_dir)) if x]
    path = os.path.join(out_dir, "r%02d_order_time.txt" % (max(taken, default=0) + 1))
    with open(path, "w") as f:
        f.write("\n".join(LINES) + "\n")
    print("written to", path)


if __name__ == "__main__":
    main()
