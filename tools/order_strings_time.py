"""Order rows by a string key on the device-resident tape, next to the host route a caller had before:
python tools/order_strings_time.py [make] [date] [screen_name] [missing10] [--out DIR]

Four documents of 1 M rows, ND, no selection (the rows are the records):
  make         configs[4]: parking-citations x1000 ND, key Make: short keys, many duplicates -- one round
  date         the same document, key IssueData: 19-byte dates that share their first bytes -- three rounds
  screen_name  the statuses of twitter.json reduced to {"id":..,"created_at":..,"user":{"screen_name":..}} and repeated to 1 M rows,
               key user.screen_name: up to 15 bytes, 100 distinct keys of 10 000 rows each
  missing10    {"id":<r>,"name":"user<5 digits>"}, 5000 names of 9 bytes -- two rounds --, one row in ten without the member: the rows
               without a key travel through both sorts
For each, alternating on the same device:
  (a) order_path_strings(key, descending, limit=10) + marshal_rows, fetched   "the 10 last by name", as text, and nothing else over PCIe
  (b) order_path_strings(key, limit=0), fetched                               the full ORDER BY: order and status of every row
  (c) extract_path_strings(key), fetched, + a stable sort on the host         the route of the parent commit (which has no way back to
      the device with the row numbers it found).  The host sort is numpy's stable argsort over the keys as fixed-width byte strings,
      built with array operations -- the fastest host route we know from Python, not sorted() over a million bytes objects
Host wall time of warmed calls; every call ends in a synchronisation.  Median of REPS runs, three medians each.  The rounds are those
of tests/order_strings_walk.max_rounds on the longest key.  The output is also written to DIR/rNN_order_strings_time.txt (DIR:
profiles/ of the repository), NN the next free number."""
import json
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

import fixtures  # noqa: E402
import sjhip  # noqa: E402
import workloads  # noqa: E402

REPS = 7
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


def document(name):
    if name == "make":
        return workloads.c5_parking_nd(1000).rstrip(b"\n"), (b"Make",)
    if name == "date":
        return workloads.c5_parking_nd(1000).rstrip(b"\n"), (b"IssueData",)
    if name == "missing10":  # synthetic: 5000 names of 9 bytes (two rounds), one row in ten without the key member
        rnd = random.Random(30)
        return "\n".join('{"id":%d}' % r if r % 10 == 9 else '{"id":%d,"name":"user%05d"}' % (r, rnd.randrange(5000)) for r in range(N)).encode(), (b"name",)
    statuses = json.loads(fixtures.load("twitter"))["statuses"]
    slim = [json.dumps({"id": s["id"], "created_at": s["created_at"], "user": {"screen_name": s["user"]["screen_name"]}}, separators=(",", ":"))
            for s in statuses]
    return "\n".join(slim[r % len(slim)] for r in range(N)).encode(), (b"user", b"screen_name")


def host_sort(off, data, st):
    """the row numbers in rank order: the OK rows by their bytes, stably, then the others in row order"""
    off = off.astype(np.int64)
    lens = np.diff(off)
    ok = np.flatnonzero(st == 0)
    width = max(int(lens.max()), 1)
    mat = np.zeros((len(lens), width), dtype=np.uint8)
    raw = np.frombuffer(data, dtype=np.uint8)
    row = np.repeat(np.arange(len(lens)), lens)
    mat[row, np.arange(len(raw)) - np.repeat(off[:-1], lens)] = raw
    keys = mat.view("S%d" % width).ravel()  # (no key of these documents holds a NUL byte, which this dtype would strip)
    return np.concatenate([ok[np.argsort(keys[ok], kind="stable")], np.flatnonzero(st != 0)])


def main():
    ctx = sjhip.Context(0)
    names = [a for a in ARGS if a in ("make", "date", "screen_name", "missing10")] or ["make", "date", "screen_name", "missing10"]
    out_dir = ARGS[ARGS.index("--out") + 1] if "--out" in ARGS else os.path.join(ROOT, "profiles")
    say(f"# {torch.cuda.get_device_name(0)}; host wall time in ms, median of {REPS} warmed calls, device-resident result, 1 M rows")
    for name in names:
        doc, key = document(name)
        d, (tl, sl) = resident(ctx, doc)

        def top10():
            ctx.select_records()
            o = ctx.order_path_strings(key, descending=True, limit=10)
            return o, ctx.marshal_rows(offsets=True)

        def full():
            ctx.select_records()
            return ctx.order_path_strings(key)

        def full_device_only():
            ctx.select_records()
            return ctx.order_path_strings(key, fetch=False)

        def host():
            off, data, st = ctx.extract_path_strings(key)
            return off, data, st, host_sort(off, data, st)

        o = full()
        off, data, st, perm = host()
        assert o.rows == len(st) and np.array_equal(o.order.astype(np.int64), perm)
        top, (n10, text, _) = top10()
        assert top.rows == 10 == n10
        lens = np.diff(off.astype(np.int64))
        longest = int(lens.max())
        keys = {data[int(a):int(b)] for a, b in zip(off[:20000], off[1:20001])}
        runs = {"a": [], "b": [], "n": [], "c": [], "e": []}
        for _ in range(3):  # alternating
            runs["a"].append(med(top10))
            runs["b"].append(med(full))
            runs["n"].append(med(full_device_only))
            runs["c"].append(med(host, reps=3))
            runs["e"].append(med(lambda: ctx.extract_path_strings(key), reps=3))
        ctx.select_records()
        m = {k: statistics.median(v) for k, v in runs.items()}
        show = lambda k: " ".join("%.3f" % x for x in runs[k])  # noqa: E731
        n = len(st)
        say(f"{name}: {len(doc)} B, tape {tl} words, {n} rows, {int((st == 0).sum())} with an OK key, key {key[-1].decode()}, longest {longest} B, "
            f"at most {longest // 7 + 1} rounds, {len(keys)} distinct keys in the first 20000 rows, {len(data)} key bytes")
        say(f"  (a) order_path_strings(limit=10, descending) + marshal_rows  {m['a']:10.3f} ms  (medians {show('a')})   PCIe {90 + len(text) + 88} B")
        say(f"  (b) order_path_strings(limit=0), fetched                     {m['b']:10.3f} ms  (medians {show('b')})   PCIe {9 * n} B")
        say(f"      order_path_strings(limit=0), not fetched                 {m['n']:10.3f} ms  (medians {show('n')})")
        say(f"  (c) extract_path_strings fetched + numpy stable argsort      {m['c']:10.3f} ms  (medians {show('c')})   (c)/(a) {m['c'] / m['a']:6.2f}  (c)/(b) {m['c'] / m['b']:6.2f}   PCIe {9 * n + 8 + len(data)} B")
        say(f"      extract_path_strings fetched, not sorted                 {m['e']:10.3f} ms  (medians {show('e')})")
        del d
    ctx.close()
    os.makedirs(out_dir, exist_ok=True)
    taken = [int(x.group(1)) for x in (re.match(r"r(\d+)", f) for f in os.listdir(out_dir)) if x]
    path = os.path.join(out_dir, "r%02d_order_strings_time.txt" % (max(taken, default=0) + 1))
    with open(path, "w") as f:
        f.write("\n".join(LINES) + "\n")
    print("written to", path)


if __name__ == "__main__":
    main()
