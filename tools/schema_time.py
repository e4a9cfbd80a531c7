"""The row schema on the device-resident tape, next to the member walk it shares and to the host walk it replaces:
python tools/schema_time.py [--copies K] [--members N] [--exp] [--profile] [--out DIR]

Three workloads, each checked against tests/schema_walk.py before anything is timed:
  parking    the parking-citations fixture K times over (NDJSON; K so that there are about a million records: few names, about
             twenty members per record), row_schema(()) on the records
  twitter    the statuses of twitter.json, K / 4 times over as lines, row_schema(("user",)) on the records' "statuses" rows
  map        the synthetic map of tools/members_time.py, {"m":{"k0":{...},...}} with N = 2^20 distinct names, row_schema(("m",)):
             every member has its own name, the election never pays
and per workload
  (s) row_schema, not fetched and fetched
  (u) unnest_members alone: the walk it shares, the floor (the selection is put back before every call, untimed)
  (h) the route without the call: the tape fetched and tests/schema_walk.py run on the host, once
  (p) with --exp, on an SJ_EXP build of the library (SJHIP_LIB=build_ab/libsjhip_exp.so): row_schema with SJHIP_SCHEMA_ELECT=E for
      E = 0 (the election compiled out: every lane probes for itself) and the other instantiations of the insert, alternating
Host wall time of warmed calls; every call ends in a synchronisation.  The variants alternate: three medians of REPS runs each; the
spread the tool reports is that of the three medians.  --profile: five calls per workload and nothing else, for
rocprofv3 --kernel-trace --stats -- python tools/schema_time.py --profile."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = sys.argv[1:]
sys.path[:0] = [os.path.join(ROOT, "simdjson-go_amd"), os.path.join(ROOT, "tests")]
import torch  # noqa: E402  (initialises its HIP runtime first, tests/conftest.py)

import fixtures  # noqa: E402
import query_walk as Q  # noqa: E402
import rows_walk as RW  # noqa: E402
import schema_walk as SW  # noqa: E402
import sjhip  # noqa: E402
import unnest_walk as UW  # noqa: E402

REPS = 9
N = int(ARGS[ARGS.index("--members") + 1]) if "--members" in ARGS else 1 << 20
EXP = "--exp" in ARGS
ROUNDS = (0, 1, 2, 4, 8, 24)  # --exp: the instantiations of k_q_schema_insert an SJ_EXP build carries


def arg(name, default):
    return int(ARGS[ARGS.index(name) + 1]) if name in ARGS else default


def med(fn, setup=None, reps=REPS):
    ts = []
    for k in range(reps + 2):
        if setup:
            setup()
        t0 = time.perf_counter()
        fn()
        if k >= 2:
            ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1e3


def spread(ms):
    return (max(ms) - min(ms)) / statistics.median(ms) * 100


def parsed(doc, nd):
    ctx = sjhip.Context(0)
    d = torch.empty(len(doc) + 256, dtype=torch.uint8, device="cuda:0")
    d[:len(doc)].copy_(torch.frombuffer(bytearray(doc), dtype=torch.uint8))
    torch.cuda.synchronize()
    tl, sl = ctx.parse_device(d.data_ptr(), len(doc), ndjson=nd, copy_strings=True)
    return ctx, d, tl, sl


def elect(e):
    if e is None:
        os.environ.pop("SJHIP_SCHEMA_ELECT", None)
    else:
        os.environ["SJHIP_SCHEMA_ELECT"] = str(e)


def workload(name, doc, nd, select, path, lines):
    ctx, dev, tl, sl = parsed(doc, nd)
    put_back = (lambda: ctx.select_rows(select)) if select is not None else ctx.select_records
    put_back()
    if "--profile" in ARGS:  # for a kernel trace: the call alone, a few times
        for _ in range(5):
            ctx.row_schema(path, fetch=False)
        ctx.close()
        return
    # the host's route, once -- and the check: fetch the tape, walk it
    t0 = time.perf_counter()
    tape, strings = ctx.fetch(tl, sl)
    t_fetch = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    w = Q.Walk(tape, strings, doc)
    rw = UW.record_rows(w) if select is None else RW.RowWalk(w, RW.select_rows(w, select)[1])
    want = SW.row_schema(rw, path)
    t_walk = (time.perf_counter() - t0) * 1e3
    for e in ((None,) + ROUNDS if EXP else (None,)):
        elect(e)
        s = ctx.row_schema(path)
        assert (s.rows, s.status.tolist(), s.members, s.names) == want[:4], (name, e)
        assert s.first_row.tolist() == want[4] and s.counts.tolist() == want[5], (name, e)
    elect(None)
    variants = [("(s) row_schema, not fetched", None, False), ("(s) row_schema, fetched", None, True)]
    if EXP:
        variants += [("(p) SJHIP_SCHEMA_ELECT=%d, not fetched" % e, e, False) for e in ROUNDS]
    times = {v[0]: [] for v in variants}
    floor = []
    for _ in range(3):  # alternating
        for label, e, fetch in variants:
            elect(e)
            times[label].append(med(lambda: ctx.row_schema(path, fetch=fetch)))
        elect(None)
        floor.append(med(lambda: ctx.unnest_members(path), setup=put_back))
        put_back()  # (unnest_members replaced the selection: row_schema runs on the one the workload names)
    fmt = lambda x: " ".join("%.3f" % v for v in x)  # noqa: E731
    lines.append(f"{name}: {len(doc)} B, tape {tl} words, {want[0]} rows, {want[2]} members, {len(want[3])} names")
    for label, _, _ in variants:
        t = times[label]
        lines.append(f"  {label:42s} {statistics.median(t):9.3f} ms  (medians {fmt(t)}; spread {spread(t):.1f} %)")
    lines.append(f"  {'(u) unnest_members alone':42s} {statistics.median(floor):9.3f} ms  (medians {fmt(floor)}; spread {spread(floor):.1f} %)")
    lines.append(f"  (h) tape fetched {t_fetch:9.1f} ms + schema_walk on the host {t_walk:9.1f} ms = {t_fetch + t_walk:9.1f} ms")
    ctx.close()


def main():
    park = fixtures.load("parking-citations").strip(b"\n")
    copies = arg("--copies", max(1, 1000000 // (park.count(b"\n") + 1)))
    tw = fixtures.load("twitter").replace(b"\n", b" ")
    lines = [f"# {torch.cuda.get_device_name(0)}; host wall time in ms, median of {REPS} warmed calls, device-resident result"
             + ("; SJ_EXP build" if EXP else "")]
    workload("parking x %d" % copies, b"\n".join([park] * copies), True, None, (), lines)
    workload("twitter x %d" % max(copies // 4, 1), b"\n".join([tw] * max(copies // 4, 1)), True, (b"statuses",), (b"user",), lines)
    map_doc = ('{"m":{' + ",".join('"k%d":{"v":%d,"s":"t%d"}' % (k, k * 7, k % 97) for k in range(N)) + "}}").encode()
    workload("map", map_doc, False, None, (b"m",), lines)
    print("\n".join(lines))
    if "--out" in ARGS:
        out_dir = ARGS[ARGS.index("--out") + 1]
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "schema_time_exp.txt" if EXP else "schema_time.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
