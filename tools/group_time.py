"""Groups on the device-resident tape, next to the host route a caller had before and to the aggregate of the same rows:
python tools/group_time.py [parking] [twitter] [synthetic] [--profile]

Three documents of 1 M rows:
  parking    configs[4]: parking-citations x1000 ND, 1 M records, no selection     key Make (a few dozen makes), value Fine FLOAT
             (every member of this document is a string, so no value converts: the walk and the reduction run, nothing is summed)
  twitter    {"statuses":[ twitter.json's 100 statuses x10000 ]} under select_rows  key user.screen_name, value retweet_count INT
             (replicated: 100 distinct names, however many rows)
  synthetic  1 M ND records {"k":"u<hex>","v":<int>}, about two thirds of the keys distinct: the high-cardinality case
For each, alternating on the same device:
  (g) group_path(key, STRING, value, kind) + fetch_groups + fetch_group_aggregates     everything the calls return, fetched
  (a) extract_path_strings(key) + extract_path(value), both fetched, grouped on the host: (a1) a Python dict, (a2) numpy.unique
      -- the route of the parent commit
  (b) aggregate_path(value, kind)                                                   the floor: one walk and one reduction
and the bytes each route moves over PCIe.  Host wall time of warmed calls; every call ends in a synchronisation.  Median of REPS
runs, three medians each (the host routes: fewer).  --profile: a few group calls only, for a kernel trace of its own."""
import json
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

import fixtures  # noqa: E402
import sjhip  # noqa: E402
import workloads  # noqa: E402

REPS = 9


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


def document(ctx, name):
    if name == "parking":
        return workloads.c5_parking_nd(1000).rstrip(b"\n"), True, None, (b"Make",), (b"Fine",), ctx.COL_FLOAT
    if name == "twitter":
        statuses = json.loads(fixtures.load("twitter"))["statuses"]
        one = ",".join(json.dumps(s, separators=(",", ":"), ensure_ascii=False) for s in statuses)
        doc = ('{"statuses":[' + ",".join([one] * 10000) + "]}").encode()
        return doc, False, (b"statuses",), (b"user", b"screen_name"), (b"retweet_count",), ctx.COL_INT
    rnd = random.Random(5)
    lines, seen = [], []
    for r in range(1000000):
        if rnd.random() < 2 / 3 or not seen:
            seen.append("u%x" % r)
            k = seen[-1]
        else:
            k = seen[rnd.randrange(len(seen))]
        lines.append('{"k":"%s","v":%d}' % (k, r & 1023))
    return "\n".join(lines).encode(), True, None, (b"k",), (b"v",), ctx.COL_INT


def main():
    ctx = sjhip.Context(0)
    names = [a for a in ARGS if a in ("parking", "twitter", "synthetic")] or ["parking", "twitter", "synthetic"]
    profile = "--profile" in ARGS
    S = ctx.COL_STRING
    print(f"# {torch.cuda.get_device_name(0)}; host wall time in ms, median of {REPS} warmed calls, device-resident result")
    for name in names:
        doc, nd, base, key, value, kind = document(ctx, name)
        d, (tl, sl) = resident(ctx, doc, nd)
        if base is not None:
            ctx.select_rows(base)

        def device():
            return ctx.group_path(key, S, value, kind)

        if profile:
            for _ in range(5):
                g = device()
            print(f"{name}: {g.rows} rows, {g.groups} groups (profile run)")
            ctx.select_records()
            del d
            continue

        def host_columns():
            off, data, st = ctx.extract_path_strings(key)
            vals, vst = ctx.extract_path(value, kind)
            return off, bytes(data), st, vals, vst

        def host_dict():
            off, data, st, vals, vst = host_columns()
            groups, order = {}, []
            o = off.tolist()
            for r in np.flatnonzero(st == ctx.COL_OK).tolist():
                k = data[o[r]:o[r + 1]]
                e = groups.get(k)
                if e is None:
                    e = groups[k] = [0, 0, 0]
                    order.append(k)
                e[0] += 1
                if vst[r] == ctx.COL_OK:
                    e[1] += 1
                    e[2] += vals[r].item()
            return order, groups

        def host_unique():
            off, data, st, vals, vst = host_columns()
            o = off.tolist()
            rows = np.flatnonzero(st == ctx.COL_OK)
            keys = np.array([data[o[r]:o[r + 1]] for r in rows.tolist()], dtype=object)
            uniq, first, inv = np.unique(keys, return_index=True, return_inverse=True)
            ok = vst[rows] == ctx.COL_OK
            return uniq, first, np.bincount(inv, minlength=len(uniq)), np.bincount(inv[ok], weights=vals[rows][ok].astype(np.float64), minlength=len(uniq))

        g = device()
        order, groups = host_dict()
        assert g.keys == order and g.group_rows.tolist() == [groups[k][0] for k in order] and g.count.tolist() == [groups[k][1] for k in order]
        if kind != ctx.COL_FLOAT:
            assert [int(x) for x in g.sum] == [groups[k][2] for k in order]
        off, data, st, vals, vst = host_columns()
        n, G = g.rows, g.groups
        pcie_g = g.key_bytes + 8 * (G + 1) + 16 * G + 5 * n + 48 * G
        pcie_a = 8 * (n + 1) + len(data) + n + 9 * n
        runs = {"g": [], "a0": [], "a1": [], "a2": [], "b": [], "n": []}
        for _ in range(3):  # alternating
            runs["g"].append(med(device))
            runs["n"].append(med(lambda: ctx.group_path(key, S, fetch=False)))
            runs["b"].append(med(lambda: ctx.aggregate_path(value, kind)))
            runs["a0"].append(med(host_columns, reps=3))
            runs["a1"].append(med(host_dict, reps=1))
            runs["a2"].append(med(host_unique, reps=1))
        m = {k: statistics.median(v) for k, v in runs.items()}
        show = lambda k: " ".join("%.3f" % x for x in runs[k])  # noqa: E731
        print(f"{name}: {len(doc)} B, tape {tl} words, {n} rows, {G} groups, {g.key_bytes} key bytes, key {key[-1].decode()} value {value[-1].decode()} kind {kind}")
        print(f"  (g)  group_path + both fetches                  {m['g']:10.3f} ms  (medians {show('g')})   PCIe {pcie_g} B")
        print(f"       group_path, no value, not fetched          {m['n']:10.3f} ms  (medians {show('n')})")
        print(f"  (a1) two columns fetched + Python dict          {m['a1']:10.3f} ms  (medians {show('a1')})   (a1)/(g) {m['a1'] / m['g']:7.2f}   PCIe {pcie_a} B")
        print(f"  (a2) two columns fetched + numpy.unique         {m['a2']:10.3f} ms  (medians {show('a2')})   (a2)/(g) {m['a2'] / m['g']:7.2f}")
        print(f"       the two columns fetched, not grouped       {m['a0']:10.3f} ms  (medians {show('a0')})   /(g)     {m['a0'] / m['g']:7.2f}")
        print(f"  (b)  aggregate_path (the floor)                 {m['b']:10.3f} ms  (medians {show('b')})   (g)/(b)  {m['g'] / m['b']:7.2f}")
        ctx.select_records()
        del d
    ctx.close()


if __name__ == "__main__":
    main()
