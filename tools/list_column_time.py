"""List columns at a path on generated ND records (1 M records, device-resident): python tools/list_column_time.py

  even    every record holds an array of 8 floats ("xs") and an array of 3 strings ("tags")
  skewed  the same total elements, half of them in 16 records (250 000 floats, 93 750 strings each)

  (a) count_where_path(path, EXISTS)                        the walk alone, 8 bytes back
  (b) extract_path_list(path, FLOAT)                        device part (the extract call) and host -> host (+ fetch)
  (c) extract_path_list_strings(path), plain and CVT        device part and host -> host
  (d) what (b) replaces: fetch_view of the whole result + find_path's indexes + a host gather of the values (numpy, vectorised)

Host wall time of warmed calls; every call ends in a synchronisation.  Median of REPS runs."""
import ctypes as C
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "simdjson-go_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402  (initialises its HIP runtime first, tests/conftest.py)

import sjhip  # noqa: E402

REPS = 15
RECORDS = 1000000
MASK = np.uint64((1 << 56) - 1)


def med(fn, reps=REPS):
    fn()
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1e3


def workload(skewed):
    rnd = random.Random(9)
    floats = ["%.6f" % rnd.uniform(-180, 180) for _ in range(4096)]
    words = ['"%s"' % "".join(rnd.choice("abcdefghij") for _ in range(rnd.randint(3, 12))) for _ in range(4096)]
    xs = lambda n: ",".join(rnd.choice(floats) for _ in range(n))
    tags = lambda n: ",".join(rnd.choice(words) for _ in range(n))
    if not skewed:
        pool = ['{"xs":[%s],"tags":[%s]}' % (xs(8), tags(3)) for _ in range(2048)]
        lines = [pool[rnd.randrange(2048)] for _ in range(RECORDS)]
    else:
        pool = ['{"xs":[%s],"tags":[%s]}' % (xs(4), tags(1 + k % 2)) for k in range(2048)]
        lines = [pool[rnd.randrange(1024) * 2 + k % 2] for k in range(RECORDS)]
        for k in range(16):
            lines[(k * 2 + 1) * RECORDS // 32] = '{"xs":[%s],"tags":[%s]}' % (xs(250000), tags(93750))
    return "\n".join(lines).encode()


def host_list(ctx, path, tl, sl):
    """(d): the whole result to the host, FindElement's indexes from the device, the floats gathered on the host"""
    L = sjhip.lib()
    tp, sp = C.c_void_p(), C.c_void_p()
    ctx._check(L.sjhip_fetch_view(ctx._h, C.byref(tp), C.byref(sp)))
    tape = np.frombuffer((C.c_uint64 * tl).from_address(tp.value), dtype=np.uint64)
    idx = ctx.find_path(*path).astype(np.int64)  # (every record has the array, and every element is a float: no checks here)
    cnt = ((tape[idx] & MASK).astype(np.int64) - idx - 2) // 2
    offs = np.zeros(len(cnt) + 1, dtype=np.int64)
    np.cumsum(cnt, out=offs[1:])
    src = np.repeat(idx + 2 - 2 * offs[:-1], cnt) + 2 * np.arange(offs[-1], dtype=np.int64)
    return offs, tape[src].view(np.float64)


def main():
    ctx = sjhip.Context(0)
    print(f"# generated ND records, {RECORDS} records, device-resident, {torch.cuda.get_device_name(0)}; host wall time in ms, "
          f"median of {REPS} warmed calls")
    for name in ("even", "skewed"):
        doc = workload(name == "skewed")
        d = torch.empty(len(doc) + 256, dtype=torch.uint8, device="cuda:0")
        d[:len(doc)].copy_(torch.frombuffer(bytearray(doc), dtype=torch.uint8))
        torch.cuda.synchronize()
        tl, sl = ctx.parse_device(d.data_ptr(), len(doc), ndjson=True, copy_strings=True)
        xs, tags = (b"xs",), (b"tags",)
        a = med(lambda: ctx.count_where_path(xs, ctx.OP_EXISTS))
        nr, ne = ctx.extract_path_list(xs, ctx.COL_FLOAT, fetch=False)
        b_dev = med(lambda: ctx.extract_path_list(xs, ctx.COL_FLOAT, fetch=False))
        b_h2h = med(lambda: ctx.extract_path_list(xs, ctx.COL_FLOAT))
        a_t = med(lambda: ctx.count_where_path(tags, ctx.OP_EXISTS))
        _, se, sb = ctx.extract_path_list_strings(tags, fetch=False)
        c_dev = med(lambda: ctx.extract_path_list_strings(tags, fetch=False))
        c_h2h = med(lambda: ctx.extract_path_list_strings(tags))
        v_dev = med(lambda: ctx.extract_path_list_strings(tags, cvt=True, fetch=False))
        v_h2h = med(lambda: ctx.extract_path_list_strings(tags, cvt=True))
        dd = med(lambda: host_list(ctx, xs, tl, sl), reps=5)
        off, vals, st = ctx.extract_path_list(xs, ctx.COL_FLOAT)
        hoff, hvals = host_list(ctx, xs, tl, sl)
        assert not st.any() and np.array_equal(hoff, off.astype(np.int64)) and np.array_equal(hvals.view(np.uint64), vals.view(np.uint64))
        print(f"{name}: {len(doc)} B, tape {tl} words; xs: {ne} floats ({ne * 8 + nr * 9 + 8} B stored); tags: {se} strings, {sb} B "
              f"({sb + se * 8 + nr * 9 + 16} B stored)")
        print(f"  (a) count_where_path EXISTS, xs / tags           {a:8.3f} / {a_t:8.3f}")
        print(f"  (b) extract_path_list FLOAT, device              {b_dev:8.3f}   {b_dev / a:5.2f}x (a)")
        print(f"      ... + fetch, host -> host                    {b_h2h:8.3f}")
        print(f"  (c) extract_path_list_strings, device            {c_dev:8.3f}   {c_dev / a_t:5.2f}x (a)")
        print(f"      ... + fetch, host -> host                    {c_h2h:8.3f}")
        print(f"      extract_path_list_strings CVT, device        {v_dev:8.3f}   {v_dev / a_t:5.2f}x (a)")
        print(f"      ... + fetch, host -> host                    {v_h2h:8.3f}")
        print(f"  (d) fetch_view + find_path + host gather (xs)    {dd:8.3f}   {dd / b_h2h:5.1f}x (b) host -> host")
        del d
    ctx.close()


if __name__ == "__main__":
    main()
