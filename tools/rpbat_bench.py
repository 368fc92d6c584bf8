#!/usr/bin/env python3
"""Cost of single-end random PBAT (walt_map_se_rpbat_batch) on the hg19-like genome: one process, one 4-strand index,
one resident batch of reads of BOTH conversions (half made C->T, half G->A by tools/synth.py's make_reads, shuffled),
timed three ways on the same batch and stream:
  * the C->T call            (walt_map_se_batch_device, ag_wildcard = 0)
  * the G->A call            (walt_map_se_batch_device, ag_wildcard = 1)
  * the random-PBAT call     (walt_map_se_rpbat_batch_device)
and a uniform sample of the batch checked against the rule of include/walt_amd.h applied to the oracle's two runs
(tests/refio.py).  The merge kernel's own time comes from running this tool under
    rocprofv3 --kernel-trace --stats -d <dir> -- python3 tools/rpbat_bench.py ...
(k_se_rpbat_merge in the kernel statistics).  Prints one JSON line.

  python3 tools/rpbat_bench.py [--reads 50000000] [--read-len 100] [--steps 3] [--warmup 1] [--sample 100000]"""
import argparse
import ctypes
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
    print("[rpbat_bench] " + msg, file=sys.stderr, flush=True)


def oracle_sample(idx, lens, bases, read_len, max_mm, b):
    """The oracle's C->T and G->A records of the sampled reads (host bases [m * read_len]); one strand of the index
    on the host at a time."""
    import refio
    import walt_amd
    orc = refio.oracle()
    cores = walt_amd.effective_cpus()
    m = bases.size // read_len
    start = np.zeros(len(lens) + 1, dtype=np.uint32)
    start[1:] = np.cumsum(lens, dtype=np.uint64).astype(np.uint32)
    offs = np.arange(m + 1, dtype=np.uint64) * read_len
    res = {}
    for ag, s0 in ((False, 0), (True, 2)):
        out = np.zeros(m, dtype=refio.best_dtype)
        orc.orc_se_init(out.ctypes.data, m, max_mm)
        work = np.zeros(1, dtype=refio.work_dtype)
        trace = np.zeros(m, dtype=refio.trace_dtype)
        for k, ch in ((0, b"+"), (1, b"-")):
            g, cnt, ix = idx.export_strand(s0 + k)
            x = refio.make_orc_strand(g, cnt, ix, start)
            orc.orc_se_map_strand_trace(ctypes.addressof(x), ch, bases.ctypes.data, offs.ctypes.data, m, int(ag), b,
                                        cores, out.ctypes.data, work.ctypes.data, trace.ctypes.data)
            del g, cnt, ix, x
        res[ag] = out
    return res[False], res[True]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=50_000_000)
    ap.add_argument("--read-len", type=int, default=100)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--genome-mbp", type=float, default=None, help="synthetic genome size (default: full scale)")
    ap.add_argument("--sample", type=int, default=100_000, help="reads of the batch the oracle checks")
    ap.add_argument("--max-mismatches", type=int, default=6)
    ap.add_argument("--bucket", type=int, default=5000)
    args = ap.parse_args()

    import torch
    import refio
    import synth
    import walt_amd
    from soak import rpbat_rule
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    scale = 1.0 if args.genome_mbp is None else args.genome_mbp * 1e6 / synth.HG19_TOTAL
    t0 = time.perf_counter()
    genome_ascii, lens, names = synth.make_genome(torch, dev, scale, seed=2, kind="hg19like")
    torch.cuda.synchronize()
    log("genome: %d bp in %d sequences (%.1f s)" % (sum(lens), len(lens), time.perf_counter() - t0))
    torch.cuda.empty_cache()
    t0 = time.perf_counter()
    idx = walt_amd.Index.build_device(genome_ascii.data_ptr(), lens, names, device=0, strands=walt_amd.STRANDS_ALL)
    log("index (4 strands): %.1f GB in HBM (%.1f s)" % (idx.device_bytes / 1e9, time.perf_counter() - t0))
    n, L = args.reads, args.read_len
    half = n // 2
    b_ct, _ = synth.make_reads(torch, dev, genome_ascii, half, L, seed=1000, ag=False)
    b_ga, _ = synth.make_reads(torch, dev, genome_ascii, n - half, L, seed=1001, ag=True)
    del genome_ascii
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    perm = torch.randperm(n, generator=gen, device=dev)
    d_bases = torch.cat([b_ct.view(half, L), b_ga.view(n - half, L)])[perm].reshape(-1).contiguous()
    truth_ga = (perm >= half)  # which reads were made A-rich (for the conv share only)
    del b_ct, b_ga
    d_off = torch.arange(n + 1, device=dev, dtype=torch.int64) * L
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    d_out = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    d_conv = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_stats = torch.zeros(4, dtype=torch.int64, device=dev)
    ws = walt_amd.se_rpbat_workspace_bytes(n, L)
    d_ws = torch.empty(ws, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    mm, b = args.max_mismatches, args.bucket

    def single(ag):
        idx.map_se_batch_device(d_bases.data_ptr(), d_off.data_ptr(), n, L, d_out.data_ptr(), d_stats.data_ptr(),
                                d_ws.data_ptr(), ws, stream=stream, ag_wildcard=ag, max_mismatches=mm, b=b)

    def rpbat():
        idx.map_se_rpbat_batch_device(d_bases.data_ptr(), d_off.data_ptr(), n, L, d_out.data_ptr(), d_conv.data_ptr(),
                                      d_stats.data_ptr(), d_ws.data_ptr(), ws, stream=stream, max_mismatches=mm, b=b)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        walt_amd.Index.check_batch(d_ws.data_ptr(), stream)
        return float(np.median(ms)), ms

    ct_ms, ct_all = timed(lambda: single(False))
    log("C->T call: %.1f ms (median of %s)" % (ct_ms, ["%.1f" % x for x in ct_all]))
    ga_ms, ga_all = timed(lambda: single(True))
    log("G->A call: %.1f ms (median of %s)" % (ga_ms, ["%.1f" % x for x in ga_all]))
    d_stats.zero_()
    rp_ms, rp_all = timed(rpbat)
    log("random-PBAT call: %.1f ms (median of %s); sum of the two: %.1f ms" % (rp_ms, ["%.1f" % x for x in rp_all],
                                                                             ct_ms + ga_ms))
    st = d_stats.cpu().numpy() // (args.warmup + args.steps)
    rec = d_out.view(torch.int32).view(n, 4)
    times = rec[:, 1]
    conv = d_conv
    share = {
        "unique": float((times == 1).float().mean()), "ambiguous": float((times >= 2).float().mean()),
        "unmapped": float((times == 0).float().mean()), "conv_A": float((conv == ord("A")).float().mean()),
        "conv_matches_how_the_read_was_made": float(((conv == ord("A")) == truth_ga).float().mean()),
    }
    log("shares: %s" % share)

    # exactness: a uniform sample against the rule on the oracle's two runs
    m = min(args.sample, n)
    sel = (torch.arange(m, device=dev, dtype=torch.int64) * n) // m
    host_bases = d_bases.view(n, L)[sel].cpu().numpy().reshape(-1).copy()
    got = d_out.view(n, 16)[sel].cpu().numpy().reshape(-1).view(walt_amd.best_match_dtype)
    got_conv = d_conv[sel].cpu().numpy()
    del d_bases, d_out, d_ws
    torch.cuda.empty_cache()
    t0 = time.perf_counter()
    c, g = oracle_sample(idx, lens, host_bases, L, mm, b)
    want, want_conv = rpbat_rule(c, g)
    same = all(np.array_equal(got[f], want[f]) for f in ("genome_pos", "times", "strand", "mismatch"))
    same = same and np.array_equal(got_conv, want_conv)
    diff = int(sum(int((got[f] != want[f]).sum()) for f in ("genome_pos", "times", "strand", "mismatch")) +
               int((got_conv != want_conv).sum()))
    log("oracle over %d sampled reads: %s (%.1f s)" % (m, "identical" if same else "%d DIFFERENCES" % diff,
                                                     time.perf_counter() - t0))
    idx.close()
    print(json.dumps({
        "tool": "rpbat_bench", "reads": n, "read_len": L, "max_mismatches": mm, "b": b,
        "genome_bp": int(sum(lens)), "steps": args.steps, "warmup": args.warmup,
        "ct_ms": ct_ms, "ga_ms": ga_ms, "rpbat_ms": rp_ms, "sum_ct_ga_ms": ct_ms + ga_ms,
        "rpbat_over_sum": rp_ms / (ct_ms + ga_ms), "ct_ms_all": ct_all, "ga_ms_all": ga_all, "rpbat_ms_all": rp_all,
        "rpbat_stats_per_call": {"too_short": int(st[0]), "probes": int(st[1]), "candidates": int(st[2]),
                                 "big_regions": int(st[3])},
        "shares": share, "oracle_sample": m, "oracle_identical": bool(same), "oracle_differences": diff,
    }))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
