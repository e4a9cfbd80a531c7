#!/usr/bin/env python3
"""bench.py -- headline benchmark of the simdjson-go Parse()/ParseND() hot path on MI355X.

Contract: `python bench.py --gpus N --steps K --warmup W` (for N>1 launched by torch.distributed.run,
one rank per GPU).  Rank 0 prints ONE JSON line.

Headline (`value`): BASELINE.json configs[1] -- twitter.json replicated 426x inside one JSON array (269 025 391 B =
256.56 MiB), stage 1 (structural index), input resident in HBM before the timed region.  A "step" is one complete
stage-1 pass over that document: the kernel (it cleans up for the next launch itself) and the structural count / verdict in
pinned host memory; the K timed steps are queued behind one another on one stream (step_mode on the line; the figure with a
synchronisation behind every step is ms_per_step_synchronised).  With N>1
every rank runs the same pass on its own replica (a single JSON document does not shard: weak scaling, no data-path
collective).

A plain run does only what that figure needs: set up, warm up, time the K steps, write the outputs if --dump-outputs DIR is
given, print the line (metric, value, unit, ms_per_step, ...).  --dump-outputs DIR: the last timed step's result as a caller of
the step receives it -- verdict and structural count (stage1_verdict_count.npy) and the structural indexes, a fixed seeded
sample of them when there are more than DUMP_SAMPLE (structural_indexes.npy, taken at structural_indexes_at.npy) -- in float64.

--full adds everything else, measured in the same run: ms_per_step_synchronised, and the objects below (all measured live in
this run unless they say "committed profile"):
  roofline      the stage-1 kernel: algorithmic bytes (N + 4*S) / average kernel time (hipEvents on the
                kernel's own stream) vs the 8 TB/s HBM3E peak; input_frac = N bytes only; read_frac = 2*FETCH_SIZE of the
                committed PMC passes / the live kernel time; at_1GiB = the same kernel on a 1.07 GB document (x1700:
                four times the Infinity Cache).
  full_parse    stage1+stage2 of the same document (tape + Strings.B left in HBM) with its own roofline object:
                algorithmic bytes of SURVEY.md 8d = (N + 4S) + (4S + N + 8T + B_str), per-kernel times from the
                committed rocprofv3 kernel trace.
  ndjson        configs[4]: parking-citations x1000 ParseND, sharded over the ranks at record boundaries (sizes and
                return codes exchanged through a shared-memory mailbox between the ranks of the node, RCCL all_gather as the
                fallback), with its roofline object; strong scaling.  At N = 1 also shard_1of8: what one of eight ranks will
                do, and the 8-GPU efficiency that projects.  ndjson_x8000: the same protocol on a 2.98 GB document.
  stream        ParseNDStream through the library (sjhip_stream_*): host memory -> tapes in host memory, 10 MiB blocks.
  query         sjhip_count_where("Make", "HOND") on the device-resident tape of configs[4]: only 8 bytes cross PCIe.
  serialize / marshal_json   Serializer.Serialize (CompressNone) and Iter.MarshalJSON of the same tape on the device.
  cpu_baseline  the oracle's AVX2 / PCLMULQDQ restatement of the reference (oracle/sjo_fast.c, kind "port": Go is not
                installed, the reference itself cannot be built) on this host in the reference's three shapes
                (BASELINE.md section 3): stage 1 on one thread, Parse() with stage 1 || stage 2 on two threads, and
                ParseNDStream's 10 MiB blocks over the host's threads; bounded samples; the reference's published
                numbers (README.md:517-557, hardware unstated) are quoted beside them.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(ROOT, "simdjson-go_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
METRIC = "GB/s parsed (stage1+stage2) + %HBM-peak, twitter.json 1GPU / parking-citations NDJSON 1-8GPU"  # BASELINE.json
PUBLISHED = {"source": "reference README.md:517-557 (Go 1.x, hardware not stated)", "unit": "GB/s",
             "parse_twitter": 1.07, "parse_canada": 0.17, "parse_twitterescaped": 0.58}
DUMP_SAMPLE = 1 << 21  # structural indexes --dump-outputs keeps (configs[1] has 23.5 M of them: 188 MB as float64)


def dump_outputs(out_dir, d_pos, ok, n):
    """--dump-outputs: the verdict, the count and the structural indexes (d_pos[:n], uint32 positions) of the last timed step as
    float64 .npy files.  Beyond DUMP_SAMPLE indexes a sample is kept, drawn with a fixed seed, so equal arguments keep equal
    positions; the positions themselves go beside it."""
    import numpy as np
    import torch
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "stage1_verdict_count.npy"), np.array([float(ok), float(n)], dtype=np.float64))
    at = np.arange(n) if n <= DUMP_SAMPLE else np.sort(np.random.default_rng(0).choice(n, DUMP_SAMPLE, replace=False))
    vals = d_pos[torch.from_numpy(at).to(d_pos.device)].cpu().numpy().view(np.uint32)
    np.save(os.path.join(out_dir, "structural_indexes.npy"), vals.astype(np.float64))
    np.save(os.path.join(out_dir, "structural_indexes_at.npy"), at.astype(np.float64))


def headline(args, world, n_bytes, s_expect, dt):
    """The line's contract fields: the K queued steps of configs[1] stage 1 (`dt` = their wall time, slowest rank)."""
    return {
        "metric": METRIC,
        "value": round(world * n_bytes / (dt / args.steps) / 1e9, 2),
        "value_is": "stage 1 only (configs[1] as BASELINE.json names it); stage1+stage2 of the same document: value_stage1_stage2 "
                    "(--full)",
        "unit": "GB/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(dt / args.steps * 1e3, 4),
        "step_mode": "queued: the K launches go behind one another on one stream, one synchronisation per 64 steps, every step's "
                     "count and verdict checked inside the timed region (sjhip_stage1_device_queue / _wait / _result)",
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "u8",
        "data": "synthetic (testdata/twitter.json replicated into one JSON array)",
        "config": {"workload": f"configs[1]: twitter.json x{args.copies} array, {n_bytes} B, stage-1 (structural index), "
                               f"one document replica per GPU", "bytes_per_gpu": n_bytes,
                   "structurals": s_expect, "parallelism": f"replicas x{world}"},
    }


def _profile(name):
    try:
        with open(os.path.join(ROOT, "profiles", name)) as f:
            return json.load(f)
    except Exception:
        return None


def live_pmc(copies=426, timeout_s=120):
    """HBM counters of the stage-1 kernel measured by THIS run: two rocprofv3 passes (FETCH_SIZE, WRITE_SIZE: they do not fit one
    pass, MI355X_MICROARCH.md) over tools/s1_time.py in a child process, only --kernel-trace beside --pmc.  -> dict with
    FETCH_SIZE_KB / WRITE_SIZE_KB (summed over the hardware instances, averaged over the dispatches of the kernel) and the kernel's
    average duration in each pass, or None (no rocprofv3, a pass failed or timed out: the committed profile is used instead)."""
    import shutil
    import sqlite3
    import subprocess
    import tempfile
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return None
    out = {}
    with tempfile.TemporaryDirectory(dir="/tmp") as tmp:
        env = dict(os.environ, COPIES=str(copies), TMPDIR="/tmp")
        for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
            env.pop(k, None)
        for counter in ("FETCH_SIZE", "WRITE_SIZE"):
            d = os.path.join(tmp, counter)
            try:
                subprocess.run([exe, "--kernel-trace", "--pmc", counter, "-d", d, "-o", "s1", "--", sys.executable,
                                os.path.join(ROOT, "tools", "s1_time.py")], cwd="/tmp", env=env, timeout=timeout_s,
                               stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=True)
                dbs = [os.path.join(r, f) for r, _, fs in os.walk(d) for f in fs if f.endswith("_results.db")]
                con = sqlite3.connect(dbs[0])
                per = {}
                for disp, val in con.execute("select dispatch_id, value from counters_collection where counter_name = ? and "
                                             "kernel_name like '%stage1_kernel%'", (counter,)):
                    per[disp] = per.get(disp, 0.0) + val
                durs = [r[0] for r in con.execute("select (end - start) / 1000.0 from kernels where name like '%stage1_kernel%'")]
                if not per or not durs:
                    return None
                out[counter + "_KB"] = sum(per.values()) / len(per)
                out["kernel_us_" + counter.lower() + "_pass"] = sum(durs) / len(durs)
                out["dispatches"] = len(per)
            except Exception:  # noqa: BLE001
                return None
    return out


def cpu_baseline():
    """BASELINE.md section 3, shapes B1 / B2 / B3 with oracle/sjo_fast.c (AVX2 + PCLMULQDQ restatement of the
    reference's assembly; stage 2 is scalar code in the reference as well).  About 20 s of CPU work."""
    import numpy as np
    import fixtures
    import oracle_lib
    import workloads
    L = oracle_lib.lib()
    nproc = os.cpu_count() or 1
    out = {"kind": "port", "unit": "GB/s", "nproc": nproc, "avx2_pclmul": bool(L.sjo_avx2_available()), "published": PUBLISHED,
           "note": "oracle/sjo_fast.c: the reference's routines restated with AVX2 / PCLMULQDQ / BMI intrinsics (bit-identical to "
                   "the scalar oracle, tests/test_oracle_fast.py); the Go + Plan-9 assembly reference cannot be built in this image"}

    def arr(b):
        return np.frombuffer(b, dtype=np.uint8)

    # B1: stage 1 only, one thread, the bench document
    doc = arr(workloads.c2_twitter_array(426))
    n = C.c_size_t(0)
    L.sjo_bench_stage1(doc.ctypes.data, 1 << 24, 0, 1, 1, C.byref(n))  # warm
    t0 = time.perf_counter()
    best = L.sjo_bench_stage1(doc.ctypes.data, doc.size, 0, 12, 1, C.byref(n))
    spent = time.perf_counter() - t0
    out["stage1_1t"] = {"value": round(doc.size / best / 1e9, 3), "cores": 1,
                        "sample": f"find_structural_bits over twitter.json x426 ({doc.size} B), best of 12 passes, {spent:.1f} s"}
    scalar = L.sjo_bench_stage1(doc.ctypes.data, 64 << 20, 0, 1, 0, C.byref(n))
    out["stage1_1t_scalar_port"] = {"value": round((64 << 20) / scalar / 1e9, 3), "cores": 1,
                                    "sample": "the byte-at-a-time restatement (oracle/sjo_stage1.c), 64 MiB, 1 pass"}
    # B1 / B2: Parse() of C1 / C3 / C4 with 1 thread and with stage 1 || stage 2 on 2 threads
    for key, name in (("twitter", "twitter"), ("canada", "canada"), ("twitterescaped", "twitterescaped")):
        d = arr(fixtures.load(name))
        for threads in (1, 2):
            rc, tl = C.c_int(0), C.c_size_t(0)
            iters = max(5, int(0.8e9 / max(d.size, 1) * 0.3))
            best = L.sjo_bench_parse(d.ctypes.data, d.size, 2, threads, min(iters, 400), C.byref(rc), C.byref(tl))
            assert rc.value == 0
            out[f"parse_{threads}t_{key}"] = {"value": round(d.size / best / 1e9, 3), "cores": threads,
                                             "sample": f"Parse({name}.json, {d.size} B), recycled buffers, best of {min(iters, 400)}"}
    # B3: ParseNDStream's shape on configs[4]
    nd = arr(workloads.c5_parking_nd(1000))
    blocks = (nd.size + (10 << 20) - 1) // (10 << 20)
    threads = max(1, min(nproc, blocks))
    failed = C.c_int(0)
    best = L.sjo_bench_nd_blocks(nd.ctypes.data, nd.size, threads, 10 << 20, 3, C.byref(failed))
    assert failed.value == 0
    out["nd_nproc"] = {"value": round(nd.size / best / 1e9, 3), "cores": threads,
                       "sample": f"parking-citations x1000 ({nd.size} B) in {blocks} blocks of 10 MiB, {threads} threads "
                                 f"(host has {nproc}), one block per thread at a time, best of 3"}
    best1 = L.sjo_bench_nd_blocks(nd.ctypes.data, 40 << 20, 1, 10 << 20, 2, C.byref(failed))
    out["nd_1t"] = {"value": round((40 << 20) / best1 / 1e9, 3), "cores": 1, "sample": "the first 40 MiB of the same, 1 thread"}
    # the contract's fields: the headline metric's CPU counterpart
    out["value"] = out["stage1_1t"]["value"]
    out["cores"] = 1
    out["sample"] = out["stage1_1t"]["sample"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--copies", type=int, default=426, help="twitter.json copies in the array (426 = 256.56 MiB)")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write the last timed step's result to DIR/<name>.npy")
    ap.add_argument("--full", action="store_true", help="also every leg beyond the headline figure (module docstring)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: no cpu_baseline")
    ap.add_argument("--stage1-only", action="store_true", help="with --full: skip every extra leg")
    args = ap.parse_args()

    import torch
    import torch.distributed as dist

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    distributed = world > 1
    if distributed:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local_rank))
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)

    import __graft_entry__ as G
    if rank == 0:
        G.build_lib()
        if args.full:
            G.build_oracle()  # cpu_baseline()
    if distributed:
        dist.barrier()
    import sjhip
    import workloads

    L = sjhip.lib()
    ctx = sjhip.Context(local_rank)

    def device_doc(doc):
        d = torch.empty(len(doc) + 256, dtype=torch.uint8, device=dev)
        d[:len(doc)].copy_(torch.frombuffer(bytearray(doc), dtype=torch.uint8))
        torch.cuda.synchronize()
        return d

    doc = workloads.c2_twitter_array(args.copies)
    n_bytes = len(doc)
    s_expect = workloads.c2_expected_structurals(args.copies)
    d_msg = device_doc(doc)
    del doc
    d_pos = torch.empty(s_expect + 1024, dtype=torch.int32, device=dev)

    def step():
        return ctx.stage1_device(d_msg.data_ptr(), n_bytes, d_pos.data_ptr(), d_pos.numel())

    for _ in range(args.warmup):
        ok, n = step()
        assert ok and n == s_expect, (ok, n, s_expect)

    def barrier():
        if distributed:
            dist.barrier()
        torch.cuda.synchronize()

    # The timed steps are QUEUED: sjhip_stage1_device_queue puts a step's launch behind the previous one on the context's
    # stream (every launch leaves count, end state and error bits in its own record of pinned host memory) and the host
    # synchronises once per batch of records -- the way the reference's ParseNDStream keeps stage 1 of the next block
    # running beside stage 2 of the previous one (simdjson_amd64.go:127-215), and what the contract's timed region (K steps
    # between two barriers) asks for.  Every step's count and verdict are checked inside the timed region.  The same K
    # steps with a synchronisation behind each (sjhip_stage1_device) are timed behind it with --full: ms_per_step_synchronised.
    QS = sjhip.Context.STAGE1_QUEUE_SLOTS

    def queued_steps(k):
        done = 0
        ok_q = n_q = None
        while done < k:
            m = min(QS, k - done)
            for slot in range(m):
                ctx.stage1_queue(d_msg.data_ptr(), n_bytes, d_pos.data_ptr(), d_pos.numel(), slot)
            ctx.stage1_wait()
            for slot in range(m):
                ok_q, n_q = ctx.stage1_result(slot, n_bytes)
                assert ok_q and n_q == s_expect, (slot, ok_q, n_q, s_expect)
            done += m
        return ok_q, n_q

    queued_steps(min(args.warmup, 2))
    barrier()
    t0 = time.perf_counter()
    ok_last, n_last = queued_steps(args.steps)
    barrier()
    dt = time.perf_counter() - t0
    if distributed:
        tmax = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dt = float(tmax.item())

    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, d_pos, ok_last, n_last)
    if not args.full:
        if rank == 0:
            print(json.dumps(headline(args, world, n_bytes, s_expect, dt)), flush=True)
        if distributed:
            dist.barrier()
            dist.destroy_process_group()
        return

    barrier()
    t1 = time.perf_counter()
    for _ in range(args.steps):
        ok, n = step()
    barrier()
    dt_sync = time.perf_counter() - t1
    assert ok and n == s_expect

    # the per-replica count gather (stands for the NDJSON tape-size exchange; 8 B per rank)
    counts = torch.tensor([n], dtype=torch.int64, device=dev)
    if distributed:
        allc = [torch.zeros_like(counts) for _ in range(world)]
        dist.all_gather(allc, counts)
        tmax = torch.tensor([dt, dt_sync], dtype=torch.float64, device=dev)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dt, dt_sync = float(tmax[0].item()), float(tmax[1].item())

    # kernel-only timing with hipEvents on the kernel's stream (rank-local)
    k_ms = ctx.stage1_time(d_msg.data_ptr(), n_bytes, d_pos.data_ptr(), d_pos.numel(), max(5, args.steps))
    algo_bytes = n_bytes + 4 * s_expect
    achieved = algo_bytes / (k_ms * 1e-3) / 1e9
    pmc = _profile("stage1_pmc.json") if args.copies == 426 else None
    roof = {"bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": round(achieved / HBM_PEAK_GBS, 4),
            "traffic": int(pmc["hbm_bytes_per_launch"]) if pmc else None,
            "kernel": "sj::stage1_kernel<1024, 2, 4, false, false>", "kernel_ms": round(k_ms, 4),
            "algorithmic_bytes": algo_bytes,
            "input_GBps": round(n_bytes / (k_ms * 1e-3) / 1e9, 1),
            "input_frac": round(n_bytes / (k_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
            "traffic_source_box": "committed profile (profiles/stage1_pmc.json), not this run: rocprofv3 PMC passes need their own runs",
            "note": "achieved = (N + 4*S) bytes / hipEvent kernel time of this run; traffic and read_frac use the HBM counters of "
                    "the committed rocprofv3 PMC passes (profiles/stage1_pmc.json: 2*FETCH_SIZE + WRITE_SIZE per launch)"}
    if pmc:
        roof["read_frac"] = round(2 * pmc["FETCH_SIZE_KB"] * 1024 / (k_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
    # ... and, on one GPU, the same counters measured by this run (two rocprofv3 PMC passes in a child process): the traffic of the
    # driver's own box replaces the committed profile's where the passes succeed
    if rank == 0 and not distributed and args.copies == 426 and not args.stage1_only and os.environ.get("SJHIP_BENCH_PMC", "1") != "0":
        live = live_pmc(426)
        if live:
            rd, wr = 2 * live["FETCH_SIZE_KB"] * 1024, live["WRITE_SIZE_KB"] * 1024
            roof["traffic"] = int(rd + wr)
            roof["traffic_read"] = int(rd)
            roof["traffic_write"] = int(wr)
            roof["traffic_source_box"] = ("this run: rocprofv3 --kernel-trace --pmc FETCH_SIZE / WRITE_SIZE (separate passes, child process, "
                                          f"{live['dispatches']} dispatches each); gfx950: FETCH_SIZE counts 64 B per 128-B request -> x2")
            roof["read_frac"] = round(rd / (k_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
            roof["read_frac_at_pmc_pass_duration"] = round(rd / (live["kernel_us_fetch_size_pass"] * 1e-6) / 1e9 / HBM_PEAK_GBS, 4)
            roof["kernel_us_in_pmc_passes"] = [round(live["kernel_us_fetch_size_pass"], 2), round(live["kernel_us_write_size_pass"], 2)]

    extra = {}
    try:
        if args.stage1_only:
            raise StopIteration

        def timed(fn, reps):
            for _ in range(3):  # (the first call of a kind grows the context's arenas, the second may grow them once more: a large
                fn()            # document is laid out for the density the context has seen, parse_api.hip)
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t) / reps
        reps = max(3, min(args.steps, 10))

        # ---- the same kernel on a document four times the Infinity Cache (rank 0 only: not part of the scaling run)
        if rank == 0 and args.copies == 426:
            big = workloads.c2_twitter_array(1700)
            nb = len(big)
            sb = workloads.c2_expected_structurals(1700)
            d_big = device_doc(big)
            del big
            p_big = torch.empty(sb + 1024, dtype=torch.int32, device=dev)
            okb, cntb = ctx.stage1_device(d_big.data_ptr(), nb, p_big.data_ptr(), p_big.numel())
            assert okb and cntb == sb
            ms_b = ctx.stage1_time(d_big.data_ptr(), nb, p_big.data_ptr(), p_big.numel(), 10)
            roof["at_1GiB"] = {"workload": f"twitter.json x1700 array, {nb} B (4x the 256 MiB Infinity Cache)", "kernel_ms": round(ms_b, 4),
                               "input_GBps": round(nb / ms_b / 1e6, 1), "achieved": round((nb + 4 * sb) / ms_b / 1e6, 1),
                               "frac": round((nb + 4 * sb) / ms_b / 1e6 / HBM_PEAK_GBS, 4),
                               "input_frac": round(nb / ms_b / 1e6 / HBM_PEAK_GBS, 4)}
            pmc_big = _profile("stage1_pmc_1GiB.json")
            if pmc_big:  # 2*FETCH_SIZE of the committed PMC pass on this document over this run's kernel time
                roof["at_1GiB"]["read_frac"] = round(2 * pmc_big["FETCH_SIZE_KB"] * 1024 / (ms_b * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
                roof["at_1GiB"]["traffic"] = int(pmc_big["hbm_bytes_per_launch"])
                roof["at_1GiB"]["traffic_source_box"] = "committed profile (profiles/stage1_pmc_1GiB.json), not this run"
            del d_big, p_big
            torch.cuda.empty_cache()

        # ---- the same kernel on a 64 MiB document: the smallest size the north_star's >= 40 % read-bandwidth target names
        if rank == 0 and args.copies == 426:
            sm = workloads.c2_twitter_array(107)
            ns = len(sm)
            ss = workloads.c2_expected_structurals(107)
            d_sm = device_doc(sm)
            del sm
            p_sm = torch.empty(ss + 1024, dtype=torch.int32, device=dev)
            oks, cnts = ctx.stage1_device(d_sm.data_ptr(), ns, p_sm.data_ptr(), p_sm.numel())
            assert oks and cnts == ss
            ms_s = ctx.stage1_time(d_sm.data_ptr(), ns, p_sm.data_ptr(), p_sm.numel(), 20)
            roof["at_64MiB"] = {"workload": f"twitter.json x107 array, {ns} B (64.4 MiB)", "kernel_ms": round(ms_s, 4),
                                "input_GBps": round(ns / ms_s / 1e6, 1), "achieved": round((ns + 4 * ss) / ms_s / 1e6, 1),
                                "frac": round((ns + 4 * ss) / ms_s / 1e6 / HBM_PEAK_GBS, 4),
                                "input_frac": round(ns / ms_s / 1e6 / HBM_PEAK_GBS, 4)}
            pmc_sm = _profile("stage1_pmc_64MiB.json")
            if pmc_sm:
                roof["at_64MiB"]["read_frac"] = round(2 * pmc_sm["FETCH_SIZE_KB"] * 1024 / (ms_s * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
                roof["at_64MiB"]["traffic"] = int(pmc_sm["hbm_bytes_per_launch"])
                roof["at_64MiB"]["traffic_source_box"] = "committed profile (profiles/stage1_pmc_64MiB.json), not this run"
            del d_sm, p_sm
            torch.cuda.empty_cache()

        # ---- stage1+stage2 of the bench document
        tl = sl = 0

        def full():
            nonlocal tl, sl
            tl, sl = ctx.parse_device(d_msg.data_ptr(), n_bytes, ndjson=False, copy_strings=True)
        t_full = timed(full, reps)
        algo_full = (n_bytes + 4 * s_expect) + (4 * s_expect + n_bytes + 8 * tl + sl)
        kprof = _profile("r06_parse_kernels.json")
        extra["full_parse"] = {
            "workload": f"configs[1] document, stage1+stage2 (tape + Strings.B left in HBM), {n_bytes} B",
            "GBps": round(n_bytes / t_full / 1e9, 2), "ms": round(t_full * 1e3, 3), "tape_words": tl, "strings_bytes": sl,
            "roofline": {"bound": "hbm", "algorithmic_bytes": algo_full, "achieved": round(algo_full / t_full / 1e9, 1),
                         "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(algo_full / t_full / 1e9 / HBM_PEAK_GBS, 4),
                         "bytes_per_input_byte": round(algo_full / n_bytes, 3),
                         "kernels_us_committed_profile": (kprof or {}).get("twitter_x426"),
                         "note": "algorithmic bytes = (N + 4S) + (4S + N + 8T + B_str), SURVEY.md 8d; time = wall time of "
                                 "sjhip_parse_device (two host syncs included); per-kernel averages: profiles/r06_parse_kernels.json"}}
        if rank == 0:  # WithCopyStrings(false): the reference publishes copy / nocopy pairs (README.md:517-557)
            tln = sln = 0

            def full_nc():
                nonlocal tln, sln
                tln, sln = ctx.parse_device(d_msg.data_ptr(), n_bytes, ndjson=False, copy_strings=False)
            t_nc = timed(full_nc, reps)
            algo_nc = (n_bytes + 4 * s_expect) + (4 * s_expect + n_bytes + 8 * tln + sln)
            extra["full_parse_nocopy"] = {
                "workload": f"configs[1] document, stage1+stage2 with WithCopyStrings(false) (only strings that unescaping changes go "
                            f"to Strings.B), {n_bytes} B", "GBps": round(n_bytes / t_nc / 1e9, 2), "ms": round(t_nc * 1e3, 3),
                "tape_words": tln, "strings_bytes": sln,
                "roofline": {"bound": "hbm", "algorithmic_bytes": algo_nc, "achieved": round(algo_nc / t_nc / 1e9, 1),
                             "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(algo_nc / t_nc / 1e9 / HBM_PEAK_GBS, 4)}}
        del d_pos

        # ---- Parse() of the single documents BASELINE.json names: configs[0] twitter.json, configs[2] canada.json
        # (number-heavy), configs[3] twitterescaped.json (escape-heavy).  host_to_host: sjhip_parse + sjhip_fetch from a
        # host buffer into host arrays (PCIe both ways, what the Go binding's Parse() costs); device: the same parse
        # with the document resident in HBM and the result left there.
        if rank == 0:
            import fixtures
            import numpy as np
            singles = {}
            for key, name in (("parse_c0_twitter", "twitter"), ("parse_c2_canada", "canada"), ("parse_c3_twitterescaped", "twitterescaped")):
                raw = fixtures.load(name).strip(b" \t\r\n")  # sjhip_parse_device takes the message as Parse() trims it
                arr = np.frombuffer(raw, dtype=np.uint8)
                pj = ctx.parse(arr)
                reuse = pj
                t_h2h = timed(lambda: ctx.parse(arr, reuse=reuse), 50)
                d_one = device_doc(raw)
                tl1 = sl1 = 0

                def one():
                    nonlocal tl1, sl1
                    tl1, sl1 = ctx.parse_device(d_one.data_ptr(), len(raw), ndjson=False, copy_strings=True)
                t_dev = timed(one, 50)
                t_h2h_nc = timed(lambda: ctx.parse(arr, reuse=reuse, copy_strings=False), 50)
                # the result read in place: Tape / Strings are views of the context's pinned block (sjhip_fetch_view),
                # the reference's `reuse` contract (overwritten by the next parse)
                t_view = timed(lambda: ctx.parse(arr, view=True), 50)

                def one_nc():
                    ctx.parse_device(d_one.data_ptr(), len(raw), ndjson=False, copy_strings=False)
                t_dev_nc = timed(one_nc, 50)
                s_one = int(ctx.stage1(arr)[1].size)
                algo = (len(raw) + 4 * s_one) + (4 * s_one + len(raw) + 8 * tl1 + sl1)
                singles[key] = {"workload": f"Parse({name}.json), {len(raw)} B, every string copied", "structurals": s_one,
                                "tape_words": tl1, "strings_bytes": sl1,
                                "host_to_host_us": round(t_h2h * 1e6, 1), "host_to_host_GBps": round(len(raw) / t_h2h / 1e9, 2),
                                "host_to_view_us": round(t_view * 1e6, 1), "host_to_view_GBps": round(len(raw) / t_view / 1e9, 2),
                                "device_us": round(t_dev * 1e6, 1), "device_GBps": round(len(raw) / t_dev / 1e9, 2),
                                "nocopy_host_to_host_us": round(t_h2h_nc * 1e6, 1), "nocopy_host_to_host_GBps": round(len(raw) / t_h2h_nc / 1e9, 2),
                                "nocopy_device_us": round(t_dev_nc * 1e6, 1), "nocopy_device_GBps": round(len(raw) / t_dev_nc / 1e9, 2),
                                "roofline": {"bound": "hbm", "algorithmic_bytes": algo, "achieved": round(algo / t_dev / 1e9, 1),
                                             "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(algo / t_dev / 1e9 / HBM_PEAK_GBS, 5),
                                             "note": "a document of this size is bound by launch and synchronisation latency, not by "
                                                     "HBM: see DESIGN.md (fixed costs per call)"}}
                del d_one
            extra["single_documents"] = singles

            # ---- many small documents in one launch set (sjhip_parse_batch_device): 256 x twitter.json resident in HBM
            one_doc = fixtures.load("twitter").strip(b" \t\r\n")
            nb_docs = 256
            blob = one_doc * nb_docs
            d_blob = device_doc(blob)
            offs_b = [k * len(one_doc) for k in range(nb_docs)]
            lens_b = [len(one_doc)] * nb_docs
            tlb = slb = 0

            def batch():
                nonlocal tlb, slb
                tlb, slb = ctx.parse_batch_device(d_blob.data_ptr(), offs_b, lens_b)
            t_batch = timed(batch, 10)
            extra["batch"] = {"workload": f"sjhip_parse_batch_device: {nb_docs} x twitter.json ({len(one_doc)} B each) resident in one "
                                          "device buffer, packed + parsed as one ND message, result left in HBM",
                              "documents": nb_docs, "bytes": len(blob), "ms": round(t_batch * 1e3, 3),
                              "GBps": round(len(blob) / t_batch / 1e9, 1), "us_per_document": round(t_batch * 1e6 / nb_docs, 2),
                              "tape_words": tlb, "strings_bytes": slb,
                              "vs_one_parse_per_document": round(singles["parse_c0_twitter"]["device_us"] * nb_docs / (t_batch * 1e6), 1)}
            del d_blob, blob

        # ---- NDJSON (configs[4]): parking-citations x1000 sharded over the ranks at record boundaries.  Each rank runs
        # phase 1 (stage 1 + measure); the ranks all_gather (tape_len, strings_len, return code) over RCCL; phase 2
        # emits tape / Strings.B with the rebased indices (tests/test_ndshard_gloo.py, tests/test_gpu_parse.py).
        from sjhip import ndshard
        nd_all = workloads.c5_parking_nd(1000)
        a, b = ndshard.record_cuts(nd_all, world)[rank]
        shard = nd_all[a:b].rstrip(b"\n")
        d_nd = device_doc(shard)
        s_nd = shard.count(b"\n") + 1

        def nd_begin():
            nonlocal tl, sl
            t_, s_ = C.c_size_t(0), C.c_size_t(0)
            ctx._check(L.sjhip_parse_shard_begin(ctx._h, C.c_void_p(d_nd.data_ptr()), len(shard), 3, C.byref(t_), C.byref(s_)))
            tl, sl = t_.value, s_.value
            return tl, sl

        def nd_finish(tape_base, strings_base, msg_base):
            ctx._check(L.sjhip_parse_shard_finish(ctx._h, tape_base, strings_base, msg_base))
            return None, None  # the tape / Strings.B stay in HBM (the bench measures the parse, not the fetch)

        def nd_gather_rccl(vals):  # 8 bytes per value and rank through RCCL: a tensor, the collective, a synchronisation
            if not distributed:
                return [tuple(vals)]
            mine = torch.tensor(list(vals), dtype=torch.int64, device=dev)
            got = [torch.zeros_like(mine) for _ in range(world)]
            dist.all_gather(got, mine)
            return [tuple(int(x) for x in g) for g in got]

        # The only exchange of the data path is 24 bytes per rank, twice per parse.  Between the ranks of one node it goes
        # through a shared-memory mailbox (sjhip.ndshard.ShmMailbox: a store and a poll, ~3 us) -- no collective launch and no
        # device synchronisation in the middle of a 100-us shard parse; RCCL is the fallback and is timed beside it.
        mailbox = ndshard.open_mailbox(rank, world, barrier=(dist.barrier if distributed else None),
                                       tag="bench%s" % os.environ.get("MASTER_PORT", str(os.getpid())))
        if distributed:  # every rank must use the same exchange
            okbox = torch.tensor([1 if mailbox is not None else 0], dtype=torch.int64, device=dev)
            dist.all_reduce(okbox, op=dist.ReduceOp.MIN)
            if int(okbox.item()) == 0 and mailbox is not None:
                mailbox.close()
                mailbox = None
        nd_gather = mailbox.gather if mailbox is not None else nd_gather_rccl

        def ndp():
            nonlocal tl, sl
            if not distributed:  # one GPU: plain ParseND of the whole document, no shard phases
                tl, sl = ctx.parse_device(d_nd.data_ptr(), len(shard), ndjson=True, copy_strings=True)
            else:  # the control flow is sjhip.ndshard's (the one the 2-rank tests run); the shard is resident in HBM
                ndshard.run_shard(rank, world, len(shard) == 0, nd_begin, nd_finish, nd_gather, a)

        if distributed:
            dist.barrier()
        t_nd = timed(ndp, reps)
        total_bytes = len(shard)
        if distributed:
            tmax = torch.tensor([t_nd], dtype=torch.float64, device=dev)
            dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
            t_nd = float(tmax.item())
            tot = torch.tensor([len(shard)], dtype=torch.int64, device=dev)
            dist.all_reduce(tot)
            total_bytes = int(tot.item())
        # the sizes of the pieces must add up to the sizes of the whole parse whichever path produced them: parking-citations
        # holds 80 tape words and 256 664 / 1000 Strings.B bytes per record in every copy (tests/test_gpu_big_nd.py closed
        # form); on one GPU the two-phase shard path (the one N > 1 runs) is run once beside the plain parse
        sizes = torch.tensor([tl, sl], dtype=torch.int64, device=dev)
        if distributed:
            dist.all_reduce(sizes)
        else:
            one = (tl, sl)
            ndshard.run_shard(0, 1, len(shard) == 0, nd_begin, nd_finish, nd_gather, 0)
            assert (tl, sl) == one, ("shard path and plain ParseND disagree", (tl, sl), one)
        assert tuple(int(x) for x in sizes) == (80000 * 1000, 256664 * 1000), tuple(int(x) for x in sizes)
        # structurals of the shard: 77 per record + one newline between records
        s_shard = 77 * s_nd + (s_nd - 1)
        algo_nd = (len(shard) + 4 * s_shard) + (4 * s_shard + len(shard) + 8 * tl + sl)
        extra["ndjson"] = {"workload": f"configs[4]: parking-citations.json x1000 ParseND, {world} shard(s) cut at record "
                                       f"boundaries, sizes + return codes exchanged between the phases", "bytes_total": total_bytes,
                           "GBps": round(total_bytes / t_nd / 1e9, 2), "ms": round(t_nd * 1e3, 3),
                           "exchange": "shared-memory mailbox (sjhip.ndshard.ShmMailbox)" if mailbox is not None else "RCCL all_gather",
                           "scaling": "strong", "tape_words_rank0": tl, "strings_bytes_rank0": sl,
                           "roofline": {"bound": "hbm", "algorithmic_bytes_rank0": algo_nd,
                                        "achieved": round(algo_nd / t_nd / 1e9, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                        "frac": round(algo_nd / t_nd / 1e9 / HBM_PEAK_GBS, 4),
                                        "bytes_per_input_byte": round(algo_nd / max(len(shard), 1), 3),
                                        "kernels_us_committed_profile": (kprof or {}).get("parking_x1000_nd"),
                                        "note": "per rank; same byte model as full_parse"}}
        if distributed and mailbox is not None:  # the same sharded parse with the RCCL exchange, for comparison
            nd_gather_used, nd_gather = nd_gather, nd_gather_rccl
            dist.barrier()
            t_rccl = timed(ndp, reps)
            tm = torch.tensor([t_rccl], dtype=torch.float64, device=dev)
            dist.all_reduce(tm, op=dist.ReduceOp.MAX)
            extra["ndjson"]["ms_with_rccl_all_gather"] = round(float(tm.item()) * 1e3, 3)
            nd_gather = nd_gather_used
        if not distributed:
            # ---- what one of EIGHT ranks will do: the first of 8 record-cut shards of configs[4] (46.6 MB) through the same
            # two-phase protocol (begin -> exchange -> finish -> exchange).  8 x its time against the whole parse on one GPU is
            # the strong-scaling efficiency an 8-GPU node can reach at best (the ranks also wait for the slowest of them).
            a8, b8 = ndshard.record_cuts(nd_all, 8)[0]
            shard8 = nd_all[a8:b8].rstrip(b"\n")
            d_s8 = device_doc(shard8)

            def s8_begin():
                t_, s_ = C.c_size_t(0), C.c_size_t(0)
                ctx._check(L.sjhip_parse_shard_begin(ctx._h, C.c_void_p(d_s8.data_ptr()), len(shard8), 3, C.byref(t_), C.byref(s_)))
                return t_.value, s_.value

            def s8_run(gather):
                ndshard.run_shard(0, 1, False, s8_begin, nd_finish, gather, 0)
            t_s8 = timed(lambda: s8_run(nd_gather), 20)
            t_s8_plain = timed(lambda: ctx.parse_device(d_s8.data_ptr(), len(shard8), ndjson=True, copy_strings=True), 20)
            extra["ndjson"]["shard_1of8"] = {
                "workload": f"the first of 8 record-cut shards of configs[4] ({len(shard8)} B) through sjhip_parse_shard_begin -> exchange "
                            f"-> sjhip_parse_shard_finish -> exchange on this GPU (what each rank of an 8-GPU run does)",
                "ms": round(t_s8 * 1e3, 4), "ms_plain_parse_of_the_shard": round(t_s8_plain * 1e3, 4),
                "exchange": extra["ndjson"]["exchange"],
                "projected_8gpu_ms": round(t_s8 * 1e3, 4), "projected_8gpu_GBps": round(total_bytes / t_s8 / 1e9, 1),
                "projected_8gpu_efficiency": round(t_nd / (8 * t_s8), 3),
                "note": "efficiency = (whole parse on one GPU) / (8 x this): an upper bound -- the ranks of a real run also wait for "
                        "the slowest of them at the exchange"}
            del d_s8
        # ---- a second ND workload, sized for eight GPUs: parking-citations x8000 (2.98 GB), strong scaling -- every rank parses
        # its 1/N of it (N = 1: the whole document on one GPU), same protocol
        if os.environ.get("SJHIP_BENCH_ND_BIG", "1") != "0":
            del d_nd
            torch.cuda.empty_cache()
            nd_big = workloads.c5_parking_nd(8000)
            ab, bb = ndshard.record_cuts(nd_big, world)[rank]
            shard_b = nd_big[ab:bb].rstrip(b"\n")
            big_total = len(nd_big) - 1
            del nd_big
            d_b = device_doc(shard_b)
            recs_b = shard_b.count(b"\n") + 1
            nb_len = len(shard_b)
            del shard_b
            tlb8 = slb8 = 0

            def b_begin():
                nonlocal tlb8, slb8
                t_, s_ = C.c_size_t(0), C.c_size_t(0)
                ctx._check(L.sjhip_parse_shard_begin(ctx._h, C.c_void_p(d_b.data_ptr()), nb_len, 3, C.byref(t_), C.byref(s_)))
                tlb8, slb8 = t_.value, s_.value
                return tlb8, slb8

            def b_run():
                ndshard.run_shard(rank, world, nb_len == 0, b_begin, nd_finish, nd_gather, ab)
            if distributed:
                dist.barrier()
            t_b = timed(b_run, 5)
            szb = torch.tensor([tlb8, slb8, recs_b], dtype=torch.int64, device=dev)
            if distributed:
                tm = torch.tensor([t_b], dtype=torch.float64, device=dev)
                dist.all_reduce(tm, op=dist.ReduceOp.MAX)
                t_b = float(tm.item())
                dist.all_reduce(szb)
            assert tuple(int(x) for x in szb) == (80000 * 8000, 256664 * 8000, 8000 * 1000), tuple(int(x) for x in szb)
            extra["ndjson_x8000"] = {"workload": f"parking-citations.json x8000 ParseND ({big_total} B), {world} shard(s) cut at record "
                                                 f"boundaries, two-phase protocol on every rank", "bytes_total": big_total,
                                     "ms": round(t_b * 1e3, 3), "GBps": round(big_total / t_b / 1e9, 2), "scaling": "strong",
                                     "exchange": extra["ndjson"]["exchange"], "tape_words_total": int(szb[0]),
                                     "strings_bytes_total": int(szb[1])}
            del d_b
            torch.cuda.empty_cache()
            ctx.trim()
            if rank == 0 and not distributed:
                d_nd = device_doc(shard)
        if mailbox is not None:
            mailbox.close()
        if rank == 0 and not distributed:
            # ---- N2: a query on the device-resident tape instead of fetching 640 MB of it
            ctx.parse_device(d_nd.data_ptr(), len(shard), ndjson=True, copy_strings=True)
            cnt = ctx.count_where(b"Make", b"HOND")
            t_q = timed(lambda: ctx.count_where(b"Make", b"HOND"), 5)
            t_f = timed(lambda: ctx.filter_where(b"Make", b"HOND", fetch=False), 3)
            nf, pjf = ctx.filter_where(b"Make", b"HOND")
            extra["query"] = {"workload": "countWhere(\"Make\", \"HOND\") over the device-resident tape of configs[4] (ndjson_test.go:250-267: "
                                          "116 per file)", "count": cnt, "expected": 116000, "count_ms": round(t_q * 1e3, 3),
                              "count_GBps_of_input": round(len(shard) / t_q / 1e9, 1),
                              "parse_plus_count_GBps": round(len(shard) / (t_nd + t_q) / 1e9, 1), "bytes_over_pcie": 8,
                              "filter_ms": round(t_f * 1e3, 3), "filter_records": nf,
                              "filter_result_bytes": int(pjf.Tape.nbytes + pjf.Strings.nbytes),
                              "full_result_bytes": int(tl * 8 + sl)}
            # ---- N3 / N4: Serializer columns and MarshalJSON of the same device-resident result
            ser = ctx.serialize(fetch=False)
            t_s = timed(lambda: ctx.serialize(fetch=False), 3)
            n_text = ctx.marshal_json(fetch=False)
            t_m = timed(lambda: ctx.marshal_json(fetch=False), 3)
            extra["serialize"] = {"workload": "Serializer.Serialize (format v3, CompressNone) of configs[4]'s tape: tag / value columns "
                                              "built on the device, Strings.B as the string column", "ms": round(t_s * 1e3, 3),
                                  "GBps_of_input": round(len(shard) / t_s / 1e9, 1), "stream_bytes": ser["stream"],
                                  "columns": {k: ser[k] for k in ("tags", "values", "strings")}}
            # ... and of a parse that left the key flags behind (SJHIP_FLAG_KEY_FLAGS: three launches less; what the parse pays)
            t_nd_kf = timed(lambda: ctx.parse_device(d_nd.data_ptr(), len(shard), ndjson=True, copy_strings=True, key_flags=True), 3)
            assert ctx.marshal_json(fetch=False) == n_text
            t_mk = timed(lambda: ctx.marshal_json(fetch=False), 3)
            extra["marshal_json"] = {"workload": "Iter.MarshalJSON of configs[4]'s tape on the device; parse with SJHIP_FLAG_KEY_FLAGS "
                                                 "(the parser leaves the key flags MarshalJSON needs)", "ms": round(t_mk * 1e3, 3),
                                     "GBps_of_input": round(len(shard) / t_mk / 1e9, 1), "text_bytes": n_text,
                                     "ms_without_key_flags": round(t_m * 1e3, 3), "parse_ms_with_key_flags": round(t_nd_kf * 1e3, 3)}
            del d_nd
            torch.cuda.empty_cache()
            # ---- N1: ParseNDStream through the library, host memory -> host memory
            import stream_bench
            hs = stream_bench.open_stream(slots=4)
            stream_bench.run(nd_all, stream=hs, copy_out=False)  # warm-up: arenas and pinned buffers at their final size
            runs = {"copy_1_thread": stream_bench.run(nd_all, stream=hs, copy_out=True, copy_threads=1),
                    "copy_4_threads": stream_bench.run(nd_all, stream=hs, copy_out=True, copy_threads=4),
                    "results_used_in_pinned_memory": stream_bench.run(nd_all, stream=hs, copy_out=False, copy_threads=4)}
            L.sjhip_stream_destroy(hs)
            # the same stream with the device-side filter (sjhip_stream_set_filter): every block is parsed and filtered
            # on the GPU, only the matching records' tape / Strings.B cross PCIe
            hf = stream_bench.open_stream(slots=4)
            assert L.sjhip_stream_set_filter(hf, b"Make", 4, b"HOND", 4) == 0
            stream_bench.run(nd_all, stream=hf, copy_out=False)
            filt = stream_bench.run(nd_all, stream=hf, copy_out=True, copy_threads=4)
            L.sjhip_stream_destroy(hf)
            filt["workload"] = "configs[4] through sjhip_stream_* with sjhip_stream_set_filter(\"Make\", \"HOND\"): host memory -> the " \
                               "matching records as (Tape, Strings.B) in host memory; H2D-bound (the results are ~5 % of the input)"
            best = dict(runs["copy_4_threads"])
            best["filtered"] = filt
            best["variants_GBps"] = {k: v["GBps"] for k, v in runs.items()}
            best["workload"] = "configs[4] through sjhip_stream_*: 10 MiB blocks read (memmove) into pinned blocks, every result copied " \
                               "out of pinned memory into the caller's arrays (PCIe-inclusive, host memory -> host memory).  One host " \
                               "thread moves ~10 GB/s, so reader and copy-out use 4 threads; the D2H of 2.4 output bytes per input " \
                               "byte bounds the pipeline near 16 GB/s on this link (variants_GBps.results_used_in_pinned_memory)"
            extra["stream"] = best
        del nd_all
    except StopIteration:
        pass
    except Exception as e:  # the headline number must still be reported
        extra["extra_error"] = repr(e)

    if rank == 0:
        line = headline(args, world, n_bytes, s_expect, dt)
        line["value_stage1_stage2"] = (extra.get("full_parse") or {}).get("GBps")
        line["step_mode"] += ("; ms_per_step_synchronised = the same K steps with a stream synchronisation behind each "
                              "(sjhip_stage1_device)")
        line["ms_per_step_synchronised"] = round(dt_sync / args.steps * 1e3, 4)
        line["value_synchronised"] = round(n_bytes * world / (dt_sync / args.steps) / 1e9, 2)
        line["config"]["workload"] += "; stage1+stage2 of the same document in full_parse, parking-citations NDJSON in ndjson"
        line["roofline"] = roof
        line.update(extra)
        if world == 1 and not args.no_cpu_baseline:
            try:
                line["cpu_baseline"] = cpu_baseline()
            except Exception as e:
                line["cpu_baseline"] = {"error": repr(e)}
        # The metric's own numbers as SCALARS inside `roofline` (records that keep only the contract's keys and the scalars
        # under them still answer "GB/s parsed (stage1+stage2)"), and once more as the last object of the line (a tail of the
        # output shows it).  `value` stays configs[1] stage 1, as BASELINE.json names that configuration.
        fp, nc, nd = extra.get("full_parse") or {}, extra.get("full_parse_nocopy") or {}, extra.get("ndjson") or {}
        sd = extra.get("single_documents") or {}
        summary = {
            "full_parse_ms": fp.get("ms"), "full_parse_GBps": fp.get("GBps"), "full_parse_frac": (fp.get("roofline") or {}).get("frac"),
            "full_parse_nocopy_ms": nc.get("ms"), "full_parse_nocopy_GBps": nc.get("GBps"),
            "ndjson_ms": nd.get("ms"), "ndjson_GBps": nd.get("GBps"), "ndjson_frac": (nd.get("roofline") or {}).get("frac"),
            "read_frac_64MiB": (roof.get("at_64MiB") or {}).get("read_frac"), "read_frac_256MiB": roof.get("read_frac"),
            "read_frac_1GiB": (roof.get("at_1GiB") or {}).get("read_frac"),
            "kernel_ms_64MiB": (roof.get("at_64MiB") or {}).get("kernel_ms"), "kernel_ms_1GiB": (roof.get("at_1GiB") or {}).get("kernel_ms"),
            "twitter_h2h_us": (sd.get("parse_c0_twitter") or {}).get("host_to_host_us"),
            "twitter_view_us": (sd.get("parse_c0_twitter") or {}).get("host_to_view_us"),
            "twitter_device_us": (sd.get("parse_c0_twitter") or {}).get("device_us"),
            "canada_h2h_us": (sd.get("parse_c2_canada") or {}).get("host_to_host_us"),
            "canada_device_us": (sd.get("parse_c2_canada") or {}).get("device_us"),
            "twitterescaped_h2h_us": (sd.get("parse_c3_twitterescaped") or {}).get("host_to_host_us"),
            "twitterescaped_device_us": (sd.get("parse_c3_twitterescaped") or {}).get("device_us"),
            "ndjson_shard_1of8_ms": ((nd.get("shard_1of8") or {}).get("ms")),
            "ndjson_projected_8gpu_efficiency": ((nd.get("shard_1of8") or {}).get("projected_8gpu_efficiency")),
            "ndjson_x8000_ms": (extra.get("ndjson_x8000") or {}).get("ms"), "ndjson_x8000_GBps": (extra.get("ndjson_x8000") or {}).get("GBps"),
            "marshal_json_ms": (extra.get("marshal_json") or {}).get("ms"),
            "stream_GBps": (extra.get("stream") or {}).get("GBps"),
        }
        for k, v in summary.items():
            roof[k] = v
        if fp.get("GBps") is not None:
            line["config"]["workload"] = (f"stage1+stage2 {fp['GBps']} GB/s ({fp['ms']} ms, frac {summary['full_parse_frac']}); ND "
                                          f"{nd.get('GBps')} GB/s; value = " + line["config"]["workload"])
        line["summary"] = summary
        print(json.dumps(line), flush=True)
    if distributed:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
