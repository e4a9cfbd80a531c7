"""Member rows on the device-resident tape, next to the same data kept as an array and to the host walk they replace:
python tools/members_time.py [--members N] [--out DIR]

Two documents of the same N records (2^20 = 1 048 576 by default, so that (e) has 65 536 objects), built here:
  the map     {"m":{"k0":{"v":0,"s":"t0"},"k1":{...},...}}              -- the collection keyed by name
  the array   {"m":[{"name":"k0","v":0,"s":"t0"},{"name":"k1",...},...]}  -- the same records with the name as a field
  (a) on the map:   unnest_members(m) + extract_row_names fetched + extract_path(v) as integers
  (b) on the array: select_rows(m) + extract_path_strings(name) fetched + extract_path(v) -- kernels this call does not share: the yardstick
  (c) the map's tape fetched and walked on the host (tests/members_walk.py), once
and, to show that the cost does not depend on the size of an object, unnest_members alone on
  (d) the map: one object of N members
  (e) {"items":[{16 members} x N/16]} under select_rows(items): N/16 objects of 16 members
Host wall time of warmed calls; every call ends in a synchronisation.  (a) and (b), and (d) and (e), alternate: three medians of
REPS runs each; the spread the tool reports is that of the three medians."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = sys.argv[1:]
sys.path[:0] = [os.path.join(ROOT, "simdjson-go_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402  (initialises its HIP runtime first, tests/conftest.py)

import members_walk as MW  # noqa: E402
import query_walk as Q  # noqa: E402
import sjhip  # noqa: E402
import unnest_walk as UW  # noqa: E402

REPS = 15
N = int(ARGS[ARGS.index("--members") + 1]) if "--members" in ARGS else 1 << 20


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


def parsed(doc):
    ctx = sjhip.Context(0)
    d = torch.empty(len(doc) + 256, dtype=torch.uint8, device="cuda:0")
    d[:len(doc)].copy_(torch.frombuffer(bytearray(doc), dtype=torch.uint8))
    torch.cuda.synchronize()
    tl, sl = ctx.parse_device(d.data_ptr(), len(doc), ndjson=False, copy_strings=True)
    return ctx, d, tl, sl


def spread(ms):
    return (max(ms) - min(ms)) / statistics.median(ms) * 100


def main():
    I = sjhip.Context.COL_INT
    map_doc = ('{"m":{' + ",".join('"k%d":{"v":%d,"s":"t%d"}' % (k, k * 7, k % 97) for k in range(N)) + "}}").encode()
    arr_doc = ('{"m":[' + ",".join('{"name":"k%d","v":%d,"s":"t%d"}' % (k, k * 7, k % 97) for k in range(N)) + "]}").encode()
    per = 16
    small_doc = ('{"items":[' + ",".join("{" + ",".join('"k%d":{"v":%d,"s":"t%d"}' % (k, k * 7, k % 97) for k in range(j, min(j + per, N))) + "}"
                                          for j in range(0, N, per)) + "]}").encode()
    cm, dm, tl, sl = parsed(map_doc)
    ca, da, _, _ = parsed(arr_doc)
    cs, ds, tls, _ = parsed(small_doc)

    def by_members():
        cm.unnest_members((b"m",))
        names = cm.extract_row_names()
        vals = cm.extract_path((b"v",), I)
        return names, vals

    def by_array():
        ca.select_rows((b"m",))
        names = ca.extract_path_strings((b"name",))
        vals = ca.extract_path((b"v",), I)
        return names, vals
    (na, va), (nb, vb) = by_members(), by_array()
    assert na[1] == nb[1] and np.array_equal(na[0], nb[0]) and np.array_equal(va[0], vb[0]) and len(va[0]) == N  # the same columns
    a, b, d, e = [], [], [], []
    for _ in range(3):  # alternating
        a.append(med(by_members, setup=cm.select_records))
        b.append(med(by_array, setup=ca.select_records))
    for _ in range(3):
        d.append(med(lambda: cm.unnest_members((b"m",)), setup=cm.select_records))
        e.append(med(lambda: cs.unnest_members(()), setup=lambda: cs.select_rows((b"items",))))
    cs.select_rows((b"items",))
    assert cs.unnest_members(())[2] == N
    # the host's route, once: fetch the tape, walk it
    t0 = time.perf_counter()
    tape, strings = cm.fetch(tl, sl)
    t_fetch = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    w = Q.Walk(tape, strings, map_doc)
    want = MW.unnest_members(UW.record_rows(w), (b"m",))
    t_walk = (time.perf_counter() - t0) * 1e3
    cm.select_records()
    records, parents, rows = cm.unnest_members((b"m",))
    assert rows == N == len(want[1]) and np.array_equal(cm.fetch_rows(records, rows)[1], np.array(want[1], dtype=np.uint64))
    assert cm.extract_row_names()[1] == b"".join(want[6])
    ma, mb, md, me = (statistics.median(x) for x in (a, b, d, e))
    fmt = lambda x: " ".join("%.3f" % v for v in x)  # noqa: E731
    lines = [f"# {torch.cuda.get_device_name(0)}; host wall time in ms, median of {REPS} warmed calls, device-resident result",
             f"{N} members; the map {len(map_doc)} B, tape {tl} words; the array {len(arr_doc)} B; names {len(na[1])} B",
             f"  (a) unnest_members(m) + extract_row_names fetched + extract_path(v)         {ma:9.3f} ms  (medians {fmt(a)}; spread {spread(a):.1f} %)",
             f"  (b) select_rows(m) + extract_path_strings(name) fetched + extract_path(v)   {mb:9.3f} ms  (medians {fmt(b)}; spread {spread(b):.1f} %)",
             f"  (a) / (b)                                                                   {ma / mb:9.2f}",
             f"  (c) tape fetched {t_fetch:9.1f} ms + walked on the host {t_walk:9.1f} ms = {t_fetch + t_walk:9.1f} ms   (c)/(a) {(t_fetch + t_walk) / ma:7.0f}",
             f"  (d) unnest_members: one object of {N} members                          {md:9.3f} ms  (medians {fmt(d)}; spread {spread(d):.1f} %)",
             f"  (e) unnest_members: {(N + per - 1) // per} objects of {per} members, tape {tls} words      {me:9.3f} ms  (medians {fmt(e)}; spread {spread(e):.1f} %)",
             f"  (d) / (e)                                                                   {md / me:9.2f}"]
    print("\n".join(lines))
    if "--out" in ARGS:
        out_dir = ARGS[ARGS.index("--out") + 1]
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "members_time.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
    for c in (cm, ca, cs):
        c.close()


if __name__ == "__main__":
    main()
