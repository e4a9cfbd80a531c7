"""queues STEPS (64) stage-1 steps on configs[1] the way bench.py's timed region does, one _wait behind them: the driver of a
`rocprofv3 --kernel-trace --stats -- python tools/s1_queue_trace.py` run, whose kernel trace shows the launches per 64
steps and their total time.  Prints the wall time per step of the queued region as well (COPIES: 426; 107 = 64 MiB)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "simdjson-go_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch, sjhip, workloads
copies = int(os.environ.get("COPIES", "426"))
steps = int(os.environ.get("STEPS", "64"))
doc = workloads.c2_twitter_array(copies)
n = len(doc)
expect = workloads.c2_expected_structurals(copies)
d_msg = torch.empty(n + 256, dtype=torch.uint8, device="cuda:0")
d_msg[:n].copy_(torch.frombuffer(bytearray(doc), dtype=torch.uint8))
d_pos = torch.empty(expect + 1024, dtype=torch.int32, device="cuda:0")
torch.cuda.synchronize()
ctx = sjhip.Context(0)
QS = sjhip.Context.STAGE1_QUEUE_SLOTS


def queued(k):
    done = 0
    while done < k:
        m = min(QS, k - done)
        for slot in range(m):
            ctx.stage1_queue(d_msg.data_ptr(), n, d_pos.data_ptr(), d_pos.numel(), slot)
        ctx.stage1_wait()
        for slot in range(m):
            ok, cnt = ctx.stage1_result(slot, n)
            assert ok and cnt == expect, (slot, ok, cnt, expect)
        done += m


queued(2)
torch.cuda.synchronize()
t0 = time.perf_counter()
queued(steps)
torch.cuda.synchronize()
ms = (time.perf_counter() - t0) * 1e3 / steps
print(f"{steps} queued steps of {n} bytes: {ms:.4f} ms per step  {n / ms / 1e6:.1f} GB/s input")
