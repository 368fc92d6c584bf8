#!/usr/bin/env python3
"""Cost of the per-cytosine pile-up (walt_meth_pileup_batch_device, walt_pileup_extract_device) beside the mapping call
it follows, on the hg19-like genome: one process, one resident batch of C->T reads (tools/synth.py's make_reads), timed
on the same batch and stream, alternating, by device events after a warm-up:
  * the mapping call alone                        (walt_map_se_batch_device)
  * mapping + calls                               (+ walt_meth_call_batch_device with calls, counts and totals)
  * mapping + calls + pile-up                     (+ walt_meth_pileup_batch_device instead: the batch read once)
  * the pile-up alone, under both shapes of the adds (option pile_rows 0 / 1; nothing but the counters written)
  * a full extraction (count, scan, write over the whole genome) and a clear.
The updates of a call are the batch totals' sum (every call of a record with times == 1).  The tool reports updates/s
against the atomic request rate the microarchitecture guide measured for float atomics (GUIDE_ATOMIC_RATE; one update
per 64-byte request is the bound it would give), sites/s, and the bytes/s of extraction and clear over the counter
bytes against the achievable streaming rate.  The table of a window of the genome is checked against the restatement in
tests/test_gpu_pileup.py, from the records of every read that reaches the window.  The kernels' own times come from
running this tool under
    rocprofv3 --kernel-trace --stats -d <dir> -- python3 tools/pileup_bench.py ...
(k_meth_pile / k_meth_pile_rows, k_pile_count, k_pile_write).  Prints one JSON line.

  python3 tools/pileup_bench.py [--reads 50000000] [--read-len 100] [--steps 10] [--warmup 2] [--window 2000000]"""
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

STREAM_RATE = 6.3e12       # bytes/s a streaming kernel can reach on the device (tools/meth_bench.py)
GUIDE_ATOMIC_RATE = 20e9   # 64-byte atomic requests/s chip-wide, measured for global float atomics


def log(msg):
    print("[pileup_bench] " + msg, file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=50_000_000)
    ap.add_argument("--read-len", type=int, default=100)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--genome-mbp", type=float, default=None, help="synthetic genome size (default: full scale)")
    ap.add_argument("--window", type=int, default=2_000_000, help="positions whose table the restatement checks")
    ap.add_argument("--max-mismatches", type=int, default=6)
    ap.add_argument("--bucket", type=int, default=5000)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()

    import torch
    import synth
    import walt_amd
    import test_gpu_pileup as rule_of
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    scale = 1.0 if args.genome_mbp is None else args.genome_mbp * 1e6 / synth.HG19_TOTAL
    t0 = time.perf_counter()
    genome_ascii, lens, names = synth.make_genome(torch, dev, scale, seed=2, kind="hg19like")
    torch.cuda.synchronize()
    glen = int(sum(lens))
    log("genome: %d bp in %d sequences (%.1f s)" % (glen, len(lens), time.perf_counter() - t0))
    torch.cuda.empty_cache()
    t0 = time.perf_counter()
    idx = walt_amd.Index.build_device(genome_ascii.data_ptr(), lens, names, device=0, strands=walt_amd.STRANDS_ALL)
    idx.enable_reference()
    torch.cuda.synchronize()
    log("index (4 strands) + reference: %.1f GB in HBM (%.1f s)" % (idx.device_bytes / 1e9, time.perf_counter() - t0))
    n, L = args.reads, args.read_len
    d_bases, _ = synth.make_reads(torch, dev, genome_ascii, n, L, seed=1000, ag=False)
    del genome_ascii
    d_off = torch.arange(n + 1, device=dev, dtype=torch.int64) * L
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    t0 = time.perf_counter()
    pile = idx.pileup()
    torch.cuda.synchronize()
    log("pile-up: %.2f GB (%.2f s to create and zero)" % (pile.device_bytes / 1e9, time.perf_counter() - t0))
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

    def calling_and_piling():
        pile.add_batch_device(d_bases.data_ptr(), d_off.data_ptr(), n, d_out.data_ptr(), 16, None, 1, "T", None,
                              d_calls.data_ptr(), d_counts.data_ptr(), d_mstats.data_ptr(), stream=stream)

    def piling():
        pile.add_batch_device(d_bases.data_ptr(), d_off.data_ptr(), n, d_out.data_ptr(), 16, None, 1, "T", stream=stream)

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(args.warmup):
        mapping()
        calling()
        calling_and_piling()
    torch.cuda.synchronize()
    t = {k: [] for k in ("map", "map_meth", "map_meth_pile", "pile_lane", "pile_rows")}
    for _ in range(args.steps):  # alternating, so that clock and temperature drift hit all legs alike
        t["map"].append(once(mapping))
        t["map_meth"].append(once(lambda: (mapping(), calling())))
        idx.set_option("pile_rows", 0)
        t["map_meth_pile"].append(once(lambda: (mapping(), calling_and_piling())))
        t["pile_lane"].append(once(piling))
        idx.set_option("pile_rows", 1)
        t["pile_rows"].append(once(piling))
        idx.set_option("pile_rows", 0)
    walt_amd.Index.check_batch(d_ws.data_ptr(), stream)
    med = {k: float(np.median(v)) for k, v in t.items()}
    log("medians of %d, ms: %s" % (args.steps, med))

    # the updates of one call: every call of a record with times == 1
    d_mstats.zero_()
    calling()
    torch.cuda.synchronize()
    mst = d_mstats.cpu().numpy()
    updates = int(mst[1:9].sum())
    del d_calls, d_counts, d_ws
    torch.cuda.empty_cache()

    # one known state for the extraction: cleared, then the batch once
    tc = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pile.clear()
        tc.append((time.perf_counter() - t0) * 1e3)
    piling()
    torch.cuda.synchronize()
    d_n = torch.zeros(3, dtype=torch.int64, device=dev)
    pile.extract_device(0, glen, None, 0, d_n.data_ptr(), d_n.data_ptr() + 8, stream=stream)  # count alone
    torch.cuda.synchronize()
    n_sites, off_m, off_u = (int(x) for x in d_n.cpu().numpy())
    d_sites = torch.empty((n_sites + 1, 16), dtype=torch.uint8, device=dev)

    def extracting():
        pile.extract_device(0, glen, d_sites.data_ptr(), n_sites + 1, d_n.data_ptr(), d_n.data_ptr() + 8, stream=stream)

    extracting()
    torch.cuda.synchronize()
    te = [once(extracting) for _ in range(max(3, args.steps // 2))]
    ext_ms, clear_ms = float(np.median(te)), float(np.median(tc))
    counter_bytes = 8 * glen
    log("updates per call %d; %d sites (off-reference %d / %d); extraction %.2f ms, clear %.2f ms" % (
        updates, n_sites, off_m, off_u, ext_ms, clear_ms))

    # exactness: the table of a window against the restatement, from the records of the reads that can reach it
    w_lo = glen // 3
    w_hi = min(glen, w_lo + args.window)
    rec = d_out.view(torch.int32).view(n, 4)
    pos = rec[:, 0].to(torch.int64) & 0xFFFFFFFF
    strands = [idx.export_strand(s)[0] for s in range(4)]
    R = [np.where(strands[2 + o] == ord("C"), np.uint8(ord("C")), strands[o]) for o in (0, 1)]
    del strands
    start = np.zeros(len(lens) + 1, dtype=np.int64)
    start[1:] = np.cumsum(lens, dtype=np.int64)
    # forward span of a read: '+' [pos, pos + L); '-' within its chromosome mirrored -- take every unique read of the
    # chromosomes the window touches whose mirrored or plain span meets it
    c_lo = int(np.searchsorted(start, w_lo, side="right")) - 1
    c_hi = int(np.searchsorted(start, w_hi - 1, side="right")) - 1
    sel = (rec[:, 1] == 1) & (pos >= int(start[c_lo])) & (pos < int(start[c_hi + 1]))
    ids = torch.nonzero(sel).flatten()
    sub_recs = d_out.view(n, 16)[ids].cpu().numpy().reshape(-1).view(walt_amd.best_match_dtype)
    sub_bases = d_bases.view(n, L)[ids].cpu().numpy()
    p = sub_recs["genome_pos"].astype(np.int64)
    c = np.searchsorted(start, p, side="right") - 1
    a = np.where(sub_recs["strand"] == b"+", p, start[c] + start[c + 1] - p - L)
    keep = np.nonzero((a < w_hi) & (a + L > w_lo))[0]
    seqs = [sub_bases[i].tobytes().decode() for i in keep]
    # (16-bit expected counters: two arrays over the whole genome stay small; a window position is covered a few times)
    acc = (np.zeros(glen, dtype=np.uint16), np.zeros(glen, dtype=np.uint16))
    meth, unmeth = rule_of.expected_counts(R, start, seqs, sub_recs[keep], "T", n_free=True, into=acc)
    for arr in (meth, unmeth):  # reads that straddle the window's ends add outside it too
        arr[:w_lo] = 0
        arr[w_hi:] = 0
    want, woff = rule_of.expected_table(R[0], start, meth, unmeth)
    got = pile.extract(w_lo, w_hi)
    identical = got[0].tobytes() == want.tobytes() and [int(got[1][0]), int(got[1][1])] == woff
    if not identical:
        log("DIFFERENCE: %d sites against %d expected, off-reference %s against %s" % (got[0].size, want.size, got[1], woff))
    log("restatement over [%d, %d): %d reads, %d sites: %s" % (w_lo, w_hi, len(seqs), got[0].size, "identical" if identical else "DIFFERENT"))
    pile.close()
    idx.close()
    line = json.dumps({
        "tool": "pileup_bench", "reads": n, "read_len": L, "max_mismatches": mm, "b": b, "genome_bp": glen,
        "steps": args.steps, "warmup": args.warmup, "pileup_bytes": int(8 * glen + (1 << 20)),
        "map_ms": med["map"], "map_plus_meth_ms": med["map_meth"], "map_plus_meth_plus_pileup_ms": med["map_meth_pile"],
        "pileup_added_to_meth_ms": med["map_meth_pile"] - med["map_meth"],
        "pileup_added_share_of_map": (med["map_meth_pile"] - med["map_meth"]) / med["map"],
        "pileup_alone_ms": {"lane_per_slice": med["pile_lane"], "neighbouring_lanes": med["pile_rows"]},
        "updates_per_call": updates,
        "updates_per_s": {"lane_per_slice": updates / (med["pile_lane"] * 1e-3), "neighbouring_lanes": updates / (med["pile_rows"] * 1e-3)},
        "guide_atomic_requests_per_s": GUIDE_ATOMIC_RATE,
        "updates_per_s_share_of_guide": {"lane_per_slice": updates / (med["pile_lane"] * 1e-3) / GUIDE_ATOMIC_RATE,
                                         "neighbouring_lanes": updates / (med["pile_rows"] * 1e-3) / GUIDE_ATOMIC_RATE},
        "sites": n_sites, "offref": [off_m, off_u], "extract_ms": ext_ms, "sites_per_s": n_sites / (ext_ms * 1e-3),
        "extract_counter_bytes_per_s": 2 * counter_bytes / (ext_ms * 1e-3),  # both passes read the counters
        "extract_share_of_achievable": 2 * counter_bytes / (ext_ms * 1e-3) / STREAM_RATE,
        "clear_ms_host_timed": clear_ms, "clear_bytes_per_s": counter_bytes / (clear_ms * 1e-3),
        "clear_share_of_achievable": counter_bytes / (clear_ms * 1e-3) / STREAM_RATE,
        "achievable_bytes_per_s": STREAM_RATE, "ms_all": t, "extract_ms_all": te, "clear_ms_all": tc,
        "window": [w_lo, w_hi], "window_reads": len(seqs), "window_sites": int(got[0].size), "window_identical": identical,
    })
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if identical else 1


if __name__ == "__main__":
    sys.exit(main())
