#!/usr/bin/env python3
"""Cost of the methylation bias table (walt_mbias_batch_device, walt_meth_pileup_batch_mbias_device) beside the calling
call it follows, on the hg19-like genome: one process, one resident batch of single-end reads (tools/synth.py's
make_reads) mapped once, then timed on the same batch and stream, alternating, by device events after a warm-up:
  * the plain calling call                 (walt_meth_call_batch_device: calls, counts and batch totals)
  * the bias kernel alone on its calls     (walt_mbias_batch_device)
  * the composition                        (walt_meth_pileup_batch_mbias_device with a null pile-up)
The bias kernel's rate is over the bytes it reads -- calls, offsets, records (no skip bytes here) -- and is put beside
the streaming rate given with --stream-rate (bytes/s, as tools/stream_calib.hip measures it on the device in the same
session) and beside the plain calling call.  The whole table is checked against the restatement of
tests/test_gpu_mbias.py's rule, evaluated on the device over all reads, and its column sums against the batch totals.
Prints one JSON line; --out also writes it to a file (profiles/mbias_hg19like.json).

  python3 tools/mbias_bench.py [--reads 50000000] [--read-len 100] [--steps 20] [--warmup 2] [--stream-rate 4.0e12]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)


def log(msg):
    print("[mbias_bench] " + msg, file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=50_000_000)
    ap.add_argument("--read-len", type=int, default=100)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--genome-mbp", type=float, default=None, help="synthetic genome size (default: full scale)")
    ap.add_argument("--max-mismatches", type=int, default=6)
    ap.add_argument("--bucket", type=int, default=5000)
    ap.add_argument("--stream-rate", type=float, default=None, help="the device's streaming rate in bytes/s (tools/stream_calib.hip)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()

    import torch
    import synth
    import walt_amd
    import test_gpu_mbias as rule_of
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    scale = 1.0 if args.genome_mbp is None else args.genome_mbp * 1e6 / synth.HG19_TOTAL
    t0 = time.perf_counter()
    genome_ascii, lens, names = synth.make_genome(torch, dev, scale, seed=2, kind="hg19like")
    torch.cuda.synchronize()
    log("genome: %d bp in %d sequences (%.1f s)" % (int(sum(lens)), len(lens), time.perf_counter() - t0))
    torch.cuda.empty_cache()
    idx = walt_amd.Index.build_device(genome_ascii.data_ptr(), lens, names, device=0, strands=walt_amd.STRANDS_ALL)
    idx.enable_reference()
    n, L = args.reads, args.read_len
    d_bases, _ = synth.make_reads(torch, dev, genome_ascii, n, L, seed=1000, ag=False)
    del genome_ascii
    d_off = torch.arange(n + 1, device=dev, dtype=torch.int64) * L
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    d_out = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    d_stats = torch.zeros(4, dtype=torch.int64, device=dev)
    d_calls = torch.zeros(n * L, dtype=torch.uint8, device=dev)
    d_counts = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    d_mstats = torch.zeros(9, dtype=torch.int64, device=dev)
    ws = walt_amd.lib().walt_se_workspace_bytes(n, L)
    d_ws = torch.empty(ws, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    idx.map_se_batch_device(d_bases.data_ptr(), d_off.data_ptr(), n, L, d_out.data_ptr(), d_stats.data_ptr(), d_ws.data_ptr(), ws,
                            stream=stream, ag_wildcard=False, max_mismatches=args.max_mismatches, b=args.bucket)
    torch.cuda.synchronize()
    walt_amd.Index.check_batch(d_ws.data_ptr(), stream)
    del d_ws
    torch.cuda.empty_cache()
    mb = walt_amd.MBias(0, 1)
    call_args = (d_bases.data_ptr(), d_off.data_ptr(), n, d_out.data_ptr(), 16, None, 1, "T", None, d_calls.data_ptr(),
                 d_counts.data_ptr(), d_mstats.data_ptr())

    def plain():
        idx.meth_call_batch_device(*call_args, stream=stream)

    def bias():
        mb.add_device(d_calls.data_ptr(), d_off.data_ptr(), n, d_out.data_ptr(), 16, stream=stream)

    def composed():
        idx.meth_call_batch_device(*call_args, stream=stream, mbias=mb, mbias_table=0)

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(args.warmup):
        plain()
        bias()
        composed()
    torch.cuda.synchronize()
    t = {"plain": [], "bias": [], "composed": []}
    for _ in range(args.steps):  # alternating, so that clock and temperature drift hit all legs alike
        t["plain"].append(once(plain))
        t["bias"].append(once(bias))
        t["composed"].append(once(composed))
    feeds = 2 * (args.warmup + args.steps)  # bias() and composed() each fed the table once per round
    got = mb.read()
    # the restatement, on the device over all reads: a record counts when times == 1 (no read is longer than 1024)
    times = d_out.view(torch.int32).view(n, 4)[:, 1]
    rows = d_calls.view(n, L)
    counted = times == 1
    want = np.zeros(rule_of.SHAPE, dtype=np.uint64)
    chunk = max(1, (1 << 28) // L)
    for b, (c, m) in rule_of.LETTERS.items():
        acc = torch.zeros(L, dtype=torch.int64, device=dev)
        for lo in range(0, n, chunk):
            acc += ((rows[lo:lo + chunk] == b) & counted[lo:lo + chunk, None]).sum(dim=0)
        want[c, m, :L] = acc.cpu().numpy().astype(np.uint64)
    identical = bool(np.array_equal(got, want * np.uint64(feeds)))
    mst = d_mstats.cpu().numpy().astype(np.uint64) // np.uint64(2 * (args.warmup + args.steps))
    m_sum, u_sum = rule_of.column_sums(want)
    sums_equal = bool(np.array_equal(m_sum, mst[1:5]) and np.array_equal(u_sum, mst[5:9]))
    log("table over %d feeds: %s; column sums %s the batch totals" % (feeds, "identical to the restatement" if identical else "DIFFERS",
                                                                      "equal" if sums_equal else "DIFFER FROM"))
    med = lambda v: float(np.median(v))
    bias_bytes = n * L + 8 * (n + 1) + 16 * n
    bias_rate = bias_bytes / (med(t["bias"]) * 1e-3)
    out = {"tool": "mbias_bench", "reads": n, "read_len": L, "genome_bp": int(sum(lens)), "steps": args.steps, "warmup": args.warmup,
           "plain_call_ms": med(t["plain"]), "plain_call_ms_min": min(t["plain"]), "plain_call_ms_max": max(t["plain"]),
           "bias_ms": med(t["bias"]), "composed_ms": med(t["composed"]), "composed_minus_plain_ms": med(t["composed"]) - med(t["plain"]),
           "bias_over_plain_call": med(t["bias"]) / med(t["plain"]), "bias_bytes": bias_bytes, "bias_bytes_per_s": bias_rate,
           "stream_bytes_per_s": args.stream_rate,
           "bias_share_of_stream": None if not args.stream_rate else bias_rate / args.stream_rate,
           "counted_reads": int(counted.sum()), "calls_counted_per_feed": int(want.sum()), "table_identical": identical,
           "column_sums_equal_totals": sums_equal, "plain_ms_all": t["plain"], "bias_ms_all": t["bias"], "composed_ms_all": t["composed"]}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    mb.close()
    idx.close()
    return 0 if identical and sums_equal else 1


if __name__ == "__main__":
    sys.exit(main())
