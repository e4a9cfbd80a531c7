"""Row predicates of several tests from one walk (where_paths), next to what a caller had before -- one where_path call per test,
or the column and a mask on the host:
python tools/where_multi_time.py

The document of tools/where_time.py: configs[4], parking-citations x1000 ND, 1 M records, no selection.
  (a) a 2-test AND      Make == "HOND" AND Color == "GY": one where_paths call against two successive where_path calls
  (b) a range           Fine >= 50 AND Fine < 100: two tests on ONE path, one call against two.  (Every value of this document is
                        a string, so both tests fail at the conversion and no row is kept: what is timed is the walk, the two
                        tests and the narrowing to nothing.)
  (c) a 4-value IN      Make in (HOND, TOYT, FORD, NISS): one where_paths call -- no sequence of where_path calls gives it --
                        against the Make column fetched and masked on the host
  (d) the count         count_where_paths of (a) and (c) against count_where_path of one test: the walk alone
The selection is put back before every timed call (select_records: not timed).

Host wall time of warmed calls; every call ends in a synchronisation.  Median of REPS runs, three medians each."""
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

REPS = 15


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


def three(fn, setup=None, reps=REPS):
    ms = [med(fn, setup, reps) for _ in range(3)]
    return statistics.median(ms), " ".join("%.3f" % x for x in ms)


def host_in(off, data, values):
    """rows whose string is one of `values`: the mask a caller builds from the fetched column"""
    starts, lens = off[:-1].astype(np.int64), np.diff(off.astype(np.int64))
    b = np.frombuffer(data, dtype=np.uint8)
    out = np.zeros(len(lens), dtype=bool)
    for value in values:
        rows = np.flatnonzero(lens == len(value))
        eq = np.ones(len(rows), dtype=bool)
        for k, ch in enumerate(value):
            eq &= b[starts[rows] + k] == ch
        out[rows[eq]] = True
    return out


def main():
    ctx = sjhip.Context(0)
    AND, OR = ctx.WHERE_AND, ctx.WHERE_OR
    doc = workloads.c5_parking_nd(1000).rstrip(b"\n")
    d = torch.empty(len(doc) + 256, dtype=torch.uint8, device="cuda:0")
    d[:len(doc)].copy_(torch.frombuffer(bytearray(doc), dtype=torch.uint8))
    torch.cuda.synchronize()
    tl, sl = ctx.parse_device(d.data_ptr(), len(doc), ndjson=True, copy_strings=True)
    back = ctx.select_records
    print(f"# {torch.cuda.get_device_name(0)}; host wall time in ms, median of {REPS} warmed calls (three medians), device-resident result")
    print(f"parking: {len(doc)} B, tape {tl} words, {ctx.count_where_path((b'Make',), ctx.OP_EXISTS)} rows")

    def versus(label, preds, program):
        def one_call():
            return ctx.where_paths(preds, program)

        def k_calls():
            for path, op, value in preds:
                got = ctx.where_path(path, op, value)
            return got

        back()
        kept = one_call()
        back()
        assert k_calls() == kept
        m1, t1 = three(one_call, back)
        mk, tk = three(k_calls, back)
        print(f"  {label}: {kept[1]} rows kept")
        print(f"      where_paths, one call, {len(preds)} tests   {m1:8.3f} ms  (medians {t1})")
        print(f"      where_path, {len(preds)} successive calls   {mk:8.3f} ms  (medians {tk})   {len(preds)} calls / one call {mk / m1:5.2f}")

    hond_gy = [((b"Make",), ctx.OP_EQ_STRING, b"HOND"), ((b"Color",), ctx.OP_EQ_STRING, b"GY")]
    versus("(a) Make == HOND AND Color == GY", hond_gy, bytes([0, 1, AND]))
    versus("(b) Fine >= 50 AND Fine < 100", [((b"Fine",), ctx.OP_GE_INT, 50), ((b"Fine",), ctx.OP_LT_INT, 100)], bytes([0, 1, AND]))

    makes = [b"HOND", b"TOYT", b"FORD", b"NISS"]
    in_preds, in_prog = [((b"Make",), ctx.OP_EQ_STRING, m) for m in makes], bytes([0, 1, OR, 2, OR, 3, OR])

    def masked():
        off, data, st = ctx.extract_path_strings((b"Make",))
        return int(host_in(off, data, makes).sum())

    back()
    kept = ctx.where_paths(in_preds, in_prog)
    back()
    assert masked() == kept[1]
    m1, t1 = three(lambda: ctx.where_paths(in_preds, in_prog), back)
    mh, th = three(masked, reps=7)
    print(f"  (c) Make in (HOND, TOYT, FORD, NISS): {kept[1]} rows kept")
    print(f"      where_paths, one call, 4 tests            {m1:8.3f} ms  (medians {t1})")
    print(f"      the Make column fetched, host mask        {mh:8.3f} ms  (medians {th})   host / device {mh / m1:5.2f}")

    back()
    c1, u1 = three(lambda: ctx.count_where_path((b"Make",), ctx.OP_EQ_STRING, b"HOND"))
    c2, u2 = three(lambda: ctx.count_where_paths(hond_gy, bytes([0, 1, AND])))
    c4, u4 = three(lambda: ctx.count_where_paths(in_preds, in_prog))
    print("  (d) the walk alone")
    print(f"      count_where_path, 1 test                  {c1:8.3f} ms  (medians {u1})")
    print(f"      count_where_paths, 2 tests on 2 paths     {c2:8.3f} ms  (medians {u2})   / 1 test {c2 / c1:5.2f}")
    print(f"      count_where_paths, 4 tests on 1 path      {c4:8.3f} ms  (medians {u4})   / 1 test {c4 / c1:5.2f}")
    del d
    ctx.close()


if __name__ == "__main__":
    main()
