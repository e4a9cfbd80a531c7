"""The three order calls of one library, for a comparison of two libraries in one session:
python tools/order_ab_time.py LABEL OUTFILE   (SJHIP_LIB chooses the library; without it, the one of this tree)

The 1 M-row configurations of tools/order_time.py (num_*: order_path), tools/order_strings_time.py (str_*: order_path_strings) and
tools/order_multi_time.py (multi_*: order_paths on both columns): the full order (limit 0), fetched and not fetched (build); nine
medians of 7 warmed calls per configuration, the two alternating.  Every line carries LABEL.  Run it once per library and process,
the libraries alternating (parent, branch, parent, branch): profiles/r30_order_one_pipeline_time.txt was made that way, the verdict
per configuration being  median(branch's medians) - median(parent's medians) <= max - min of the parent's medians."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LABEL, OUT = sys.argv[1], sys.argv[2]
sys.argv = sys.argv[:1]
sys.path[:0] = [os.path.join(ROOT, "simdjson-go_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import torch  # noqa: E402
import sjhip  # noqa: E402
import order_time as OT  # noqa: E402
import order_strings_time as ST  # noqa: E402
import order_multi_time as MT  # noqa: E402

LINES = []


def say(text):
    print(text, flush=True)
    LINES.append(text)
    with open(OUT, "w") as f:
        f.write("\n".join(LINES) + "\n")


def med(fn, reps=7):
    ts = []
    for k in range(reps + 2):
        t0 = time.perf_counter()
        fn()
        if k >= 2:
            ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1e3


def measure(ctx, name, call):
    def fetched():
        ctx.select_records()
        return call(True)

    def build():
        ctx.select_records()
        return call(False)

    runs = {"fetched": [], "build": []}
    for _ in range(9):
        runs["fetched"].append(med(fetched))
        runs["build"].append(med(build))
    ctx.select_records()
    for k in ("fetched", "build"):
        v = runs[k]
        say("%s %-28s median %8.4f min %8.4f max %8.4f spread %7.4f  medians %s" % (
            LABEL, name + "_" + k, statistics.median(v), min(v), max(v), max(v) - min(v), " ".join("%.4f" % x for x in v)))


def main():
    ctx = sjhip.Context(0)
    say("# %s: %s; %s; ms, 9 medians of 7 warmed calls, 1 M rows" % (LABEL, os.environ.get("SJHIP_LIB", "the library of this commit"),
                                                                     torch.cuda.get_device_name(0)))
    docs = {}

    def doc_of(key, make):
        if key not in docs:
            docs.clear()
            docs[key] = make()
        return docs[key]

    jobs = []
    for name in ("digits3", "digits8", "missing10"):
        jobs.append(("num_" + name, ("num", name), lambda name=name: OT.document(ctx, name)))
    for name in ("screen_name", "missing10"):
        jobs.append(("str_" + name, ("str", name), lambda name=name: ST.document(name)))
    for name in ("few", "unique"):
        jobs.append(("multi_" + name, ("multi", name), lambda name=name: MT.document(name)))
    park = lambda: (OT.workloads.c5_parking_nd(1000).rstrip(b"\n"),)  # noqa: E731
    jobs.append(("num_parking", ("parking",), park))
    jobs.append(("str_make", ("parking",), park))
    jobs.append(("str_date", ("parking",), park))
    jobs.append(("multi_parking", ("parking",), park))
    d = None
    held = None
    for label, key, make in jobs:
        got = doc_of(key, make)
        if held != key:
            d = None
            d, _ = OT.resident(ctx, got[0])
            held = key
        if label.startswith("num_"):
            path, kind = ((b"Fine",), ctx.COL_FLOAT) if label == "num_parking" else (got[1], got[2])
            call = lambda fetch, path=path, kind=kind: ctx.order_path(path, kind, fetch=fetch)  # noqa: E731
        elif label.startswith("str_"):
            path = {"str_make": (b"Make",), "str_date": (b"IssueData",)}.get(label) or got[1]
            call = lambda fetch, path=path: ctx.order_path_strings(path, fetch=fetch)  # noqa: E731
        else:
            cols = [((b"Make",), MT.S, False), ((b"Color",), MT.S, False)] if label == "multi_parking" else got[1]
            call = lambda fetch, cols=cols: ctx.order_paths(cols, fetch=fetch)  # noqa: E731
        measure(ctx, label, call)
    ctx.close()


if __name__ == "__main__":
    main()
