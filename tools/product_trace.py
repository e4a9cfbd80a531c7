"""One call of every product that is built on the device and fetched later, once on a whole result and once on a sharded one:
rocprofv3 --kernel-trace --memory-copy-trace -d DIR -- python tools/product_trace.py
python tools/product_trace.py --summarize DIR OUT    (kernel dispatches per name, copies per direction, and the ordered kernel
                                                      names of the whole-result half: what a host-side refactor must leave alone)

The document is the one of tests/test_gpu_product_parts.py (~1.2 MiB, five shards of which one holds no value).  Per half: string
column extract + fetch, list extract + fetch for numbers, strings and CVT, table extract + fetch of every column.  A marker
kernel of torch (a fill) separates the halves in the trace."""
import glob
import os
import sqlite3
import sys
from collections import Counter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "simdjson-go_amd"), os.path.join(ROOT, "tests")]


def products(ctx):
    ctx.extract_path_strings((b"s",))
    ctx.extract_path_list((b"n",), ctx.COL_FLOAT)
    ctx.extract_path_list_strings((b"t",))
    ctx.extract_path_list_strings((b"t",), cvt=True)
    ctx.extract_table([((b"x",), ctx.COL_INT), ((b"s",), ctx.COL_STRING), ((b"s",), ctx.COL_STRING_CVT), ((b"id",), ctx.COL_FLOAT)])


def run():
    import torch  # (initialises its HIP runtime first, tests/conftest.py)
    torch.cuda.init()
    import fixtures
    import sjhip
    import test_gpu_product_parts as P
    doc = P.ABC
    one, many = sjhip.Context(0), sjhip.Context(0)
    one.parse(doc, ndjson=True)
    with fixtures.nd_shard_limits(P.LIMIT, P.SHARD):
        many.parse(doc, ndjson=True)
    mark = torch.empty(4096, dtype=torch.int32, device="cuda:0")
    for ctx in (one, many):
        mark.fill_(7)  # the marker: the products of `one` lie between the first and the second fill of the trace
        torch.cuda.synchronize()
        products(ctx)
    one.close()
    many.close()


def summarize(root, out):
    dbs = sorted(glob.glob(os.path.join(root, "**", "*_results.db"), recursive=True))
    assert len(dbs) == 1, dbs
    cur = sqlite3.connect(dbs[0]).cursor()
    names = [n for (n,) in cur.execute("select name from kernels order by start")]
    copies = Counter(n for (n,) in cur.execute("select name from memory_copies"))
    ours = lambda n: "k_q_" in n or "k_tw_" in n
    fills = [i for i, n in enumerate(names) if "fill" in n.lower() and "rocclr" not in n]
    lines = [f"# kernels: {len(names)} dispatches, {len(set(names))} names"]
    lines += [f"{c:6d}  {n[:150]}" for n, c in sorted(Counter(names).items())]
    lines.append(f"# copies: {sum(copies.values())}")
    lines += [f"{c:6d}  {n}" for n, c in sorted(copies.items())]
    if len(fills) >= 2:
        lines.append("# the whole-result half (one stream): query kernels in order of their start")
        lines += [f"        {n.split('(')[2].split(')')[-1].lstrip(':') if n.startswith('(anonymous') else n.split('(')[0]}"
                  for n in names[fills[-2]:fills[-1]] if ours(n)]
    else:
        lines.append(f"# (the marker fills were not found: {len(fills)})")
    text = "\n".join(lines) + "\n"
    open(out, "w").write(text)
    print(text)


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2], sys.argv[3])
    else:
        run()
