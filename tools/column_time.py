"""Columns at a path on configs[4] (parking-citations x1000 ND, 1 M records, device-resident): python tools/column_time.py

  (a) count_where_path(path, EXISTS)                                  the walk alone, 8 bytes back
  (b) extract_path(path, INT)                                         the same walk + 9 bytes per record back (all TYPE here:
                                                                      the parking values are strings)
  (c) extract_path_strings(path, cvt=True) + fetch                    device part (the extract call) and host -> host (+ fetch)
  (d) what (c) replaces: fetch_view of the whole result + find_path's indexes + a host gather of the strings (numpy, vectorised)

Host wall time of warmed calls; every call ends in a synchronisation.  Median of REPS runs."""
import ctypes as C
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
MASK, SBIT = np.uint64((1 << 56) - 1), np.uint64(1 << 55)


def med(fn, reps=REPS):
    fn()
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1e3


def host_column(ctx, path, tl, sl):
    """(d): the whole result to the host, FindElement's indexes from the device, the strings gathered on the host"""
    L = sjhip.lib()
    tp, sp = C.c_void_p(), C.c_void_p()
    ctx._check(L.sjhip_fetch_view(ctx._h, C.byref(tp), C.byref(sp)))
    tape = np.frombuffer((C.c_uint64 * tl).from_address(tp.value), dtype=np.uint64)
    strings = np.frombuffer((C.c_uint8 * sl).from_address(sp.value), dtype=np.uint8)
    idx = ctx.find_path(*path)
    hit = idx < np.uint64(ctx.PATH_NOT_OBJECT)
    v = idx[hit].astype(np.int64)
    words = tape[v]
    ok = (words >> np.uint64(56)) == np.uint64(ord('"'))
    starts = (words[ok] & MASK & ~SBIT).astype(np.int64)  # (copy mode: every string is in Strings.B)
    lens = tape[v[ok] + 1].astype(np.int64)
    offs = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    src = np.repeat(starts - offs[:-1], lens) + np.arange(offs[-1], dtype=np.int64)
    return offs, strings[src].tobytes()


def main():
    doc = workloads.c5_parking_nd(1000).rstrip(b"\n")
    ctx = sjhip.Context(0)
    d = torch.empty(len(doc) + 256, dtype=torch.uint8, device="cuda:0")
    d[:len(doc)].copy_(torch.frombuffer(bytearray(doc), dtype=torch.uint8))
    torch.cuda.synchronize()
    tl, sl = ctx.parse_device(d.data_ptr(), len(doc), ndjson=True, copy_strings=True)
    print(f"# configs[4]: parking-citations x1000 ND, {len(doc)} B, tape {tl} words, Strings.B {sl} B, device-resident, "
          f"{torch.cuda.get_device_name(0)}; host wall time, median of {REPS} warmed calls")
    for path in ((b"Make",), (b"Latitude",)):
        p = "/".join(k.decode() for k in path)
        a = med(lambda: ctx.count_where_path(path, ctx.OP_EXISTS))
        b = med(lambda: ctx.extract_path(path, ctx.COL_INT))
        nr, nb = ctx.extract_path_strings(path, cvt=True, fetch=False)
        c_dev = med(lambda: ctx.extract_path_strings(path, cvt=True, fetch=False))
        c_h2h = med(lambda: ctx.extract_path_strings(path, cvt=True))
        dd = med(lambda: host_column(ctx, path, tl, sl), reps=5)
        off, data, st = ctx.extract_path_strings(path, cvt=True)
        hoff, hdata = host_column(ctx, path, tl, sl)
        assert hdata == data and np.array_equal(hoff, off[np.r_[0, np.nonzero(st == 0)[0] + 1]].astype(np.int64)), p
        print(f"{p:9s} records {nr}  column bytes {nb}")
        print(f"  (a) count_where_path EXISTS            {a:8.3f} ms")
        print(f"  (b) extract_path INT                   {b:8.3f} ms   {b / a:5.2f}x (a)")
        print(f"  (c) extract_path_strings CVT, device   {c_dev:8.3f} ms")
        print(f"      ... + fetch, host -> host          {c_h2h:8.3f} ms")
        print(f"  (d) fetch_view + find_path + host gather {dd:6.3f} ms   {dd / c_h2h:5.1f}x (c) host -> host")
    ctx.close()


if __name__ == "__main__":
    main()
