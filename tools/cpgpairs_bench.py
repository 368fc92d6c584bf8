#!/usr/bin/env python3
"""Cost of the adjacent-CpG pair table (walt_cpgpairs_*, walt_meth_pileup_batch_pairs_device) on the hg19-like genome: one
process, one resident batch of single-end reads (tools/synth.py's make_reads) mapped once, then
  * the build of the rank structure          (walt_cpgpairs_create: bitmap, directory, zeroed table; wall clock, it waits)
and, timed on the same batch and stream, alternating, by device events after a warm-up:
  * the plain calling call                   (walt_meth_call_batch_device: calls, counts and batch totals)
  * the bias kernel alone on its calls       (walt_mbias_batch_device: it streams the same bytes)
  * the pair kernel alone on its calls       (walt_cpgpairs_batch_device)
  * the composition                          (walt_meth_pileup_batch_pairs_device with a null pile-up)
  * the extraction of the whole genome       (walt_cpgpairs_extract_device: count, scan, write)
The pair kernel's rate is over the bytes it streams -- calls, offsets, records (no skip bytes here); what it gathers from
the bitmap and the directory per call comes on top and is not counted.  Checks: n_pairs against a scan of the genome on
the device; the table of a sample of the reads, fed to a second table, against a restatement that finds the pairs in each
read's own window of the genome and walks its calls in order (tests/test_gpu_cpgpairs.py's rule, keyed by position).
Prints one JSON line; --out also writes it to a file (profiles/cpgpairs_hg19like.json).

  python3 tools/cpgpairs_bench.py [--reads 50000000] [--read-len 100] [--steps 20] [--warmup 2] [--sample 20000]"""
import argparse
import bisect
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
    print("[cpgpairs_bench] " + msg, file=sys.stderr, flush=True)


def count_pairs(torch, genome_ascii, starts):
    """C followed by G inside one chromosome, over the whole genome on the device"""
    n, total, piece = genome_ascii.numel(), 0, 1 << 28
    for lo in range(0, n - 1, piece):
        hi = min(lo + piece, n - 1)
        total += int(((genome_ascii[lo:hi] == ord("C")) & (genome_ascii[lo + 1:hi + 1] == ord("G"))).sum())
    ends = torch.tensor([s - 1 for s in starts[1:-1]], device=genome_ascii.device, dtype=torch.int64)
    if ends.numel():
        total -= int(((genome_ascii[ends] == ord("C")) & (genome_ascii[ends + 1] == ord("G"))).sum())
    return total


def sample_table(genome_ascii, starts, calls, L, rec):
    """{pos: [next, MM, MU, UM, UU]} of the reads of a sample, each walked in its own window of the genome"""
    out = {}
    glen = starts[-1]
    for r in range(rec.size):
        p = int(rec["genome_pos"][r])
        if int(rec["times"][r]) != 1 or p >= glen:
            continue
        k = bisect.bisect_right(starts, p) - 1
        lo, hi = starts[k], starts[k + 1]
        minus = rec["strand"][r] == b"-"
        f_of = (lambda i: lo + hi - 1 - (p + i)) if minus else (lambda i: p + i)
        w_lo = max(lo, min(f_of(0), f_of(L - 1)) - 1)
        w_hi = min(hi, max(f_of(0), f_of(L - 1)) + 2)
        text = genome_ascii[w_lo:w_hi].cpu().numpy().tobytes()
        pairs = [w_lo + c for c in range(len(text) - 1) if text[c:c + 2] == b"CG"]  # (the window ends inside the chromosome)
        number = {c: j for j, c in enumerate(pairs)}
        prev = None
        for i, b in enumerate(calls[r * L:(r + 1) * L].tolist()):
            if b not in (0x7A, 0x5A) or p + i >= hi:
                continue
            f = f_of(i)
            j = number.get(f, number.get(f - 1))
            if j is None:
                continue
            cur = (j, 1 if b == 0x7A else 0)
            if prev is not None and abs(cur[0] - prev[0]) == 1:
                (jl, ul), (jh, uh) = sorted([prev, cur])
                row = out.setdefault(pairs[jl], [pairs[jh], 0, 0, 0, 0])
                row[1 + 2 * ul + uh] += 1
            prev = cur
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=50_000_000)
    ap.add_argument("--read-len", type=int, default=100)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sample", type=int, default=20000, help="reads of the checked sample")
    ap.add_argument("--genome-mbp", type=float, default=None, help="synthetic genome size (default: full scale)")
    ap.add_argument("--max-mismatches", type=int, default=6)
    ap.add_argument("--bucket", type=int, default=5000)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()

    import torch
    import synth
    import walt_amd
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    scale = 1.0 if args.genome_mbp is None else args.genome_mbp * 1e6 / synth.HG19_TOTAL
    t0 = time.perf_counter()
    genome_ascii, lens, names = synth.make_genome(torch, dev, scale, seed=2, kind="hg19like")
    torch.cuda.synchronize()
    starts = [0]
    for v in lens:
        starts.append(starts[-1] + int(v))
    log("genome: %d bp in %d sequences (%.1f s)" % (starts[-1], len(lens), time.perf_counter() - t0))
    torch.cuda.empty_cache()
    idx = walt_amd.Index.build_device(genome_ascii.data_ptr(), lens, names, device=0, strands=walt_amd.STRANDS_ALL)
    idx.enable_reference()
    n, L = args.reads, args.read_len
    d_bases, _ = synth.make_reads(torch, dev, genome_ascii, n, L, seed=1000, ag=False)
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

    # the rank structure: built twice, the second build timed (the first pays for the kernels' load)
    idx.cpg_pairs().close()
    t0 = time.perf_counter()
    pairs = idx.cpg_pairs()
    build_ms = (time.perf_counter() - t0) * 1e3
    n_pairs = pairs.n_pairs
    want_pairs = count_pairs(torch, genome_ascii, starts)
    log("rank structure: %d pairs (%d by the scan), %d bytes, built in %.1f ms" % (n_pairs, want_pairs, pairs.device_bytes, build_ms))
    mb = walt_amd.MBias(0, 1)
    call_args = (d_bases.data_ptr(), d_off.data_ptr(), n, d_out.data_ptr(), 16, None, 1, "T", None, d_calls.data_ptr(),
                 d_counts.data_ptr(), d_mstats.data_ptr())
    d_n = torch.zeros(1, dtype=torch.int64, device=dev)

    def plain():
        idx.meth_call_batch_device(*call_args, stream=stream)

    def bias():
        mb.add_device(d_calls.data_ptr(), d_off.data_ptr(), n, d_out.data_ptr(), 16, stream=stream)

    def pair():
        pairs.add_device(d_calls.data_ptr(), d_off.data_ptr(), n, d_out.data_ptr(), 16, stream=stream)

    def composed():
        idx.meth_call_batch_device(*call_args, stream=stream, pairs=pairs)

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
        pair()
        composed()
    torch.cuda.synchronize()
    t = {"plain": [], "bias": [], "pair": [], "composed": [], "extract": []}
    for _ in range(args.steps):  # alternating, so that clock and temperature drift hit all legs alike
        t["plain"].append(once(plain))
        t["bias"].append(once(bias))
        t["pair"].append(once(pair))
        t["composed"].append(once(composed))
    feeds = 2 * (args.warmup + args.steps)  # pair() and composed() each fed the table once per round

    # the extraction of the whole genome: the count first, then into an array of exactly that size
    glen = starts[-1]
    pairs.extract_device(0, glen, None, 0, d_n.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    entries = int(d_n.item())
    d_sites = torch.zeros(max(entries, 1) * 24, dtype=torch.uint8, device=dev)
    for k in range(args.warmup + args.steps):
        ms = once(lambda: pairs.extract_device(0, glen, d_sites.data_ptr(), entries, d_n.data_ptr(), stream=stream))
        if k >= args.warmup:
            t["extract"].append(ms)
    sites = d_sites.cpu().numpy()[:entries * 24].view(walt_amd.cpgpair_site_dtype)
    couples_per_feed = int(sites["n"].astype(np.uint64).sum()) // feeds
    ascending = bool((np.diff(sites["pos"].astype(np.int64)) > 0).all() and (sites["next"] > sites["pos"]).all())
    divisible = bool((sites["n"] % feeds == 0).all())  # every feed added the same couples

    # a sample of the reads through a second table, against the restatement in each read's own window
    k = min(args.sample, n)
    check = idx.cpg_pairs()
    check.add_device(d_calls.data_ptr(), d_off.data_ptr(), k, d_out.data_ptr(), 16, stream=stream)
    torch.cuda.synchronize()
    got = {int(s["pos"]): [int(s["next"])] + [int(v) for v in s["n"]] for s in check.extract()}
    rec = d_out[:k * 16].cpu().numpy().view(walt_amd.best_match_dtype)
    want = sample_table(genome_ascii, starts, d_calls[:k * L].cpu().numpy(), L, rec)
    sample_ok = got == want
    log("table: %d entries, %d couples per feed, %s; sample of %d reads: %d entries, %s" %
        (entries, couples_per_feed, "ascending" if ascending else "NOT ASCENDING", k, len(want),
         "identical to the restatement" if sample_ok else "DIFFERS"))
    check.close()

    med = lambda v: float(np.median(v))
    stream_bytes = n * L + 8 * (n + 1) + 16 * n
    extract_bytes = glen // 8 + glen // 32 + 16 * n_pairs + 24 * entries
    out = {"tool": "cpgpairs_bench", "reads": n, "read_len": L, "genome_bp": glen, "steps": args.steps, "warmup": args.warmup,
           "n_pairs": n_pairs, "n_pairs_by_scan": want_pairs, "device_bytes": int(pairs.device_bytes), "rank_build_ms": build_ms,
           "plain_call_ms": med(t["plain"]), "plain_call_ms_min": min(t["plain"]), "plain_call_ms_max": max(t["plain"]),
           "bias_ms": med(t["bias"]), "pair_ms": med(t["pair"]), "composed_ms": med(t["composed"]),
           "composed_minus_plain_ms": med(t["composed"]) - med(t["plain"]), "pair_over_plain_call": med(t["pair"]) / med(t["plain"]),
           "pair_over_bias": med(t["pair"]) / med(t["bias"]), "streamed_bytes": stream_bytes,
           "pair_bytes_per_s": stream_bytes / (med(t["pair"]) * 1e-3), "bias_bytes_per_s": stream_bytes / (med(t["bias"]) * 1e-3),
           "extract_ms": med(t["extract"]), "extract_entries": entries, "extract_bytes": extract_bytes,
           "extract_bytes_per_s": extract_bytes / (med(t["extract"]) * 1e-3), "extract_pairs_per_s": n_pairs / (med(t["extract"]) * 1e-3),
           "couples_per_feed": couples_per_feed, "feeds": feeds, "entries_ascending": ascending, "counts_divisible_by_feeds": divisible,
           "sample_reads": k, "sample_entries": len(want), "sample_identical": bool(sample_ok),
           "plain_ms_all": t["plain"], "bias_ms_all": t["bias"], "pair_ms_all": t["pair"], "composed_ms_all": t["composed"],
           "extract_ms_all": t["extract"]}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ok = n_pairs == want_pairs and ascending and divisible and sample_ok
    pairs.close()
    mb.close()
    idx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
