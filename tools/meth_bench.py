#!/usr/bin/env python3
"""Cost of the methylation calls (walt_meth_call_batch_device) beside the mapping call they follow, on the hg19-like
genome: one process, one resident batch of C->T reads (tools/synth.py's make_reads), timed two ways on the same batch
and stream, alternating, by device events after a warm-up:
  * the mapping call alone                     (walt_map_se_batch_device)
  * the mapping call followed by the calling   (+ walt_meth_call_batch_device with calls, counts and totals)
and the calling alone.  The index is built on the device with all four strands and the reference is made from them
(walt_index_enable_reference); the reference arrays and the kernel are those of an index opened with the C->T strands
and WALT_WITH_REFERENCE.  The tool computes the bytes the kernel must move from the batch's shapes (bases, offsets,
records, calls, counts, reference words touched; strictly and in whole 128-byte lines) and reports bytes/s against
the achievable streaming rate, and checks a uniform sample of the batch against the restatement of the contract in
tests/test_gpu_meth.py.  The kernel's own time comes from running this tool under
    rocprofv3 --kernel-trace --stats -d <dir> -- python3 tools/meth_bench.py ...
(k_meth_call in the kernel statistics).  Prints one JSON line.

  python3 tools/meth_bench.py [--reads 50000000] [--read-len 100] [--steps 20] [--warmup 2] [--sample 100000]"""
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

STREAM_RATE = 6.3e12  # bytes/s a streaming kernel can reach on the device (the figure bench.py's traffic leg uses)


def log(msg):
    print("[meth_bench] " + msg, file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=50_000_000)
    ap.add_argument("--read-len", type=int, default=100)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--genome-mbp", type=float, default=None, help="synthetic genome size (default: full scale)")
    ap.add_argument("--sample", type=int, default=100_000, help="reads of the batch the restatement checks")
    ap.add_argument("--max-mismatches", type=int, default=6)
    ap.add_argument("--bucket", type=int, default=5000)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()

    import torch
    import synth
    import walt_amd
    import test_gpu_meth as rule_of
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
    bytes_before = idx.device_bytes
    t1 = time.perf_counter()
    idx.enable_reference()
    torch.cuda.synchronize()
    ref_s = time.perf_counter() - t1
    ref_bytes = idx.device_bytes - bytes_before
    log("index (4 strands): %.1f GB in HBM (%.1f s); reference: %.2f GB more, built in %.3f s" % (
        bytes_before / 1e9, t1 - t0, ref_bytes / 1e9, ref_s))
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
    mm, b = args.max_mismatches, args.bucket

    def mapping():
        idx.map_se_batch_device(d_bases.data_ptr(), d_off.data_ptr(), n, L, d_out.data_ptr(), d_stats.data_ptr(),
                                d_ws.data_ptr(), ws, stream=stream, ag_wildcard=False, max_mismatches=mm, b=b)

    def calling():
        idx.meth_call_batch_device(d_bases.data_ptr(), d_off.data_ptr(), n, d_out.data_ptr(), 16, None, 1, "T", None,
                                   d_calls.data_ptr(), d_counts.data_ptr(), d_mstats.data_ptr(), stream=stream)

    def both():
        mapping()
        calling()

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(args.warmup):
        both()
    torch.cuda.synchronize()
    map_all, both_all, call_all = [], [], []
    for _ in range(args.steps):  # alternating, so that clock and temperature drift hit all three alike
        map_all.append(once(mapping))
        both_all.append(once(both))
        call_all.append(once(calling))
    walt_amd.Index.check_batch(d_ws.data_ptr(), stream)
    map_ms, both_ms, call_ms = (float(np.median(x)) for x in (map_all, both_all, call_all))
    log("mapping %.2f ms, mapping + calling %.2f ms (+%.2f), calling alone %.2f ms (medians of %d)" % (
        map_ms, both_ms, both_ms - map_ms, call_ms, args.steps))

    # the bytes the kernel must move, from the batch's shapes
    rec = d_out.view(torch.int32).view(n, 4)
    pos, times = rec[:, 0].to(torch.int64) & 0xFFFFFFFF, rec[:, 1]
    mapped = times != 0
    first, last = torch.clamp(pos - 2, min=0) >> 4, (pos + L + 1) >> 4
    ref_words = int(((last - first + 1) * mapped).sum())
    ref_lines = int((((last >> 5) - (first >> 5) + 1) * mapped).sum())
    n_mapped = int(mapped.sum())
    fixed = n * L + 8 * (n + 1) + 16 * n + n * L + 16 * n  # bases, offsets, records, calls, counts
    # (an unmapped read's bases are not read: its calls are all '.')
    strict = fixed - (n - n_mapped) * L + 4 * ref_words
    lines = fixed - (n - n_mapped) * L + 128 * ref_lines
    traffic = {
        "bases": n_mapped * L, "offsets": 8 * (n + 1), "records": 16 * n, "calls": n * L, "counts": 16 * n,
        "reference_strict": 4 * ref_words, "reference_whole_lines": 128 * ref_lines,
        "total_strict": strict, "total_whole_lines": lines,
        "strict_bytes_per_s": strict / (call_ms * 1e-3), "whole_lines_bytes_per_s": lines / (call_ms * 1e-3),
        "achievable_bytes_per_s": STREAM_RATE,
        "share_of_achievable_strict": strict / (call_ms * 1e-3) / STREAM_RATE,
        "share_of_achievable_whole_lines": lines / (call_ms * 1e-3) / STREAM_RATE,
    }
    log("traffic: %.2f GB strictly, %.2f GB in whole lines: %.2f / %.2f TB/s = %.0f %% / %.0f %% of %.1f TB/s" % (
        strict / 1e9, lines / 1e9, traffic["strict_bytes_per_s"] / 1e12, traffic["whole_lines_bytes_per_s"] / 1e12,
        100 * traffic["share_of_achievable_strict"], 100 * traffic["share_of_achievable_whole_lines"], STREAM_RATE / 1e12))
    mst = d_mstats.cpu().numpy() // (args.warmup + 2 * args.steps)
    totals = {"reads": int(mst[0]), "meth": [int(x) for x in mst[1:5]], "unmeth": [int(x) for x in mst[5:9]]}
    log("totals per call: %s" % totals)

    # exactness: a uniform sample against the restatement on the strand genomes
    m = min(args.sample, n)
    sel = (torch.arange(m, device=dev, dtype=torch.int64) * n) // m
    host_bases = d_bases.view(n, L)[sel].cpu().numpy()
    got_recs = d_out.view(n, 16)[sel].cpu().numpy().reshape(-1).view(walt_amd.best_match_dtype)
    got_calls = d_calls.view(n, L)[sel].cpu().numpy()
    got_counts = d_counts.view(n, 16)[sel].cpu().numpy().reshape(-1).view(walt_amd.meth_counts_dtype)
    del d_bases, d_out, d_ws, d_calls, d_counts
    torch.cuda.empty_cache()
    t0 = time.perf_counter()
    strands = [idx.export_strand(s)[0] for s in range(4)]
    R = [np.where(strands[2 + o] == ord("C"), np.uint8(ord("C")), strands[o]) for o in (0, 1)]
    del strands
    start = np.zeros(len(lens) + 1, dtype=np.int64)
    start[1:] = np.cumsum(lens, dtype=np.int64)
    diff = 0
    for i in range(m):
        seq = host_bases[i].tobytes().decode()
        r = got_recs[i]
        want, wc = rule_of.expected_read(R, start, seq, r["genome_pos"], r["times"], bytes(r["strand"]), "T")
        gc = got_counts[i]["meth"].tolist() + got_counts[i]["unmeth"].tolist()
        if got_calls[i].tobytes().decode("latin-1") != want or gc != wc:
            diff += 1
    log("restatement over %d sampled reads: %s (%.1f s)" % (m, "identical" if diff == 0 else "%d DIFFERENCES" % diff,
                                                           time.perf_counter() - t0))
    idx.close()
    line = json.dumps({
        "tool": "meth_bench", "reads": n, "read_len": L, "max_mismatches": mm, "b": b, "genome_bp": int(sum(lens)),
        "steps": args.steps, "warmup": args.warmup, "reference_bytes": int(ref_bytes), "reference_build_s": ref_s,
        "map_ms": map_ms, "map_plus_meth_ms": both_ms, "meth_added_ms": both_ms - map_ms, "meth_alone_ms": call_ms,
        "meth_added_share_of_map": (both_ms - map_ms) / map_ms,
        "map_ms_all": map_all, "map_plus_meth_ms_all": both_all, "meth_alone_ms_all": call_all,
        "mapped_share": n_mapped / n, "traffic": traffic, "totals_per_call": totals,
        "sample": m, "sample_identical": diff == 0, "sample_differences": diff,
    })
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if diff == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
