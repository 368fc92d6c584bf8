#!/usr/bin/env python3
"""Cost of the four-CpG epiallele table (walt_epialleles_*, walt_meth_pileup_batch_epi_device) on the hg19-like genome: one
process, one resident batch of single-end reads (tools/synth.py's make_reads) mapped once, then
  * the build of the object                  (walt_epialleles_create: bitmap, directory, zeroed table; wall clock, it waits)
and, timed on the same batch and stream, alternating, by device events after a warm-up:
  * the plain calling call                   (walt_meth_call_batch_device: calls, counts and batch totals)
  * the pair kernel alone on its calls       (walt_cpgpairs_batch_device: the yardstick, same gathers per call)
  * the window kernel alone on its calls     (walt_epialleles_batch_device)
  * the composition                          (walt_meth_pileup_batch_epi_device with a null pile-up and no pair table)
  * the extraction of the whole genome       (walt_epialleles_extract_device: count, scan, write) at min_total 1 and 10
Checks: n_pairs against the pair table's; every feed added the same windows; the table of a sample of the reads, fed to a
second table, against a restatement that finds the pairs in each read's own window of the genome and takes every four
calls that follow each other (tests/test_gpu_epialleles.py's rule, keyed by position).
Prints one JSON line; --out also writes it to a file (profiles/epialleles_hg19like.json).

  python3 tools/epialleles_bench.py [--reads 50000000] [--read-len 100] [--steps 20] [--warmup 2] [--sample 20000]"""
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
    print("[epialleles_bench] " + msg, file=sys.stderr, flush=True)


def sample_table(genome_ascii, starts, calls, L, rec):
    """{pos: [last, n0 .. n15]} of the reads of a sample, each walked in its own window of the genome"""
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
        seen = []
        for i, b in enumerate(calls[r * L:(r + 1) * L].tolist()):
            if b not in (0x7A, 0x5A) or p + i >= hi:
                continue
            f = f_of(i)
            j = number.get(f, number.get(f - 1))
            if j is not None:
                seen.append((j, 1 if b == 0x7A else 0))
        for t in range(len(seen) - 3):
            four = seen[t:t + 4]
            for s in (1, -1):
                if all(four[i][0] == four[0][0] + i * s for i in (1, 2, 3)):
                    fwd = four if s == 1 else four[::-1]
                    row = out.setdefault(pairs[fwd[0][0]], [pairs[fwd[3][0]]] + [0] * 16)
                    row[1 + 8 * fwd[0][1] + 4 * fwd[1][1] + 2 * fwd[2][1] + fwd[3][1]] += 1
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

    # the object: built twice, the second build timed (the first pays for the kernels' load)
    idx.epialleles().close()
    t0 = time.perf_counter()
    epi = idx.epialleles()
    build_ms = (time.perf_counter() - t0) * 1e3
    pairs = idx.cpg_pairs()
    n_pairs = epi.n_pairs
    log("object: %d pairs (the pair table: %d), %d bytes, built in %.1f ms" % (n_pairs, pairs.n_pairs, epi.device_bytes, build_ms))
    call_args = (d_bases.data_ptr(), d_off.data_ptr(), n, d_out.data_ptr(), 16, None, 1, "T", None, d_calls.data_ptr(),
                 d_counts.data_ptr(), d_mstats.data_ptr())
    d_n = torch.zeros(1, dtype=torch.int64, device=dev)

    def plain():
        idx.meth_call_batch_device(*call_args, stream=stream)

    def pair():
        pairs.add_device(d_calls.data_ptr(), d_off.data_ptr(), n, d_out.data_ptr(), 16, stream=stream)

    def window():
        epi.add_device(d_calls.data_ptr(), d_off.data_ptr(), n, d_out.data_ptr(), 16, stream=stream)

    def composed():
        idx.meth_call_batch_device(*call_args, stream=stream, epi=epi)

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(args.warmup):
        plain()
        pair()
        window()
        composed()
    torch.cuda.synchronize()
    t = {"plain": [], "pair": [], "window": [], "composed": [], "extract1": [], "extract10": []}
    for _ in range(args.steps):  # alternating, so that clock and temperature drift hit all legs alike
        t["plain"].append(once(plain))
        t["pair"].append(once(pair))
        t["window"].append(once(window))
        t["composed"].append(once(composed))
    feeds = 2 * (args.warmup + args.steps)  # window() and composed() each fed the table once per round

    # every feed added the same windows: the whole table once, untimed
    glen = starts[-1]
    epi.extract_device(0, glen, 1, None, 0, d_n.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    fed = int(d_n.item())
    d_sites = torch.zeros(max(fed, 1) * 72, dtype=torch.uint8, device=dev)
    epi.extract_device(0, glen, 1, d_sites.data_ptr(), fed, d_n.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    sites = d_sites.cpu().numpy()[:fed * 72].view(walt_amd.epiallele_site_dtype)
    del d_sites
    # the extraction of the whole genome from the table of one feed (what a run holds after this batch): the count first,
    # then into an array of exactly that size
    epi.clear()
    window()
    torch.cuda.synchronize()
    entries = {}
    for m in (1, 10):
        epi.extract_device(0, glen, m, None, 0, d_n.data_ptr(), stream=stream)
        torch.cuda.synchronize()
        entries[m] = int(d_n.item())
        d_sites = torch.zeros(max(entries[m], 1) * 72, dtype=torch.uint8, device=dev)
        for k in range(args.warmup + args.steps):
            ms = once(lambda: epi.extract_device(0, glen, m, d_sites.data_ptr(), entries[m], d_n.data_ptr(), stream=stream))
            if k >= args.warmup:
                t["extract%d" % m].append(ms)
        del d_sites
    windows_per_feed = int(sites["n"].astype(np.uint64).sum()) // feeds
    ascending = bool((np.diff(sites["pos"].astype(np.int64)) > 0).all() and (sites["last"] > sites["pos"]).all())
    divisible = bool((sites["n"] % feeds == 0).all())  # every feed added the same windows
    span_max = int((sites["last"].astype(np.int64) - sites["pos"].astype(np.int64)).max()) if fed else 0

    # a sample of the reads through a second table, against the restatement in each read's own window
    k = min(args.sample, n)
    check = idx.epialleles()
    check.add_device(d_calls.data_ptr(), d_off.data_ptr(), k, d_out.data_ptr(), 16, stream=stream)
    torch.cuda.synchronize()
    got = {int(s["pos"]): [int(s["last"])] + [int(v) for v in s["n"]] for s in check.extract()}
    rec = d_out[:k * 16].cpu().numpy().view(walt_amd.best_match_dtype)
    want = sample_table(genome_ascii, starts, d_calls[:k * L].cpu().numpy(), L, rec)
    sample_ok = got == want
    log("table: %d entries (%d with 10 reads), %d windows per feed, %s; sample of %d reads: %d entries, %s" %
        (entries[1], entries[10], windows_per_feed, "ascending" if ascending else "NOT ASCENDING", k, len(want),
         "identical to the restatement" if sample_ok else "DIFFERS"))
    check.close()

    med = lambda v: float(np.median(v))
    stream_bytes = n * L + 8 * (n + 1) + 16 * n
    out = {"tool": "epialleles_bench", "reads": n, "read_len": L, "genome_bp": glen, "steps": args.steps, "warmup": args.warmup,
           "n_pairs": n_pairs, "n_pairs_of_pair_table": pairs.n_pairs, "device_bytes": int(epi.device_bytes),
           "pair_table_device_bytes": int(pairs.device_bytes), "build_ms": build_ms,
           "plain_call_ms": med(t["plain"]), "pair_ms": med(t["pair"]), "window_ms": med(t["window"]), "composed_ms": med(t["composed"]),
           "window_ms_min": min(t["window"]), "window_ms_max": max(t["window"]), "pair_ms_min": min(t["pair"]), "pair_ms_max": max(t["pair"]),
           "composed_minus_plain_ms": med(t["composed"]) - med(t["plain"]), "window_over_pair": med(t["window"]) / med(t["pair"]),
           "window_over_plain_call": med(t["window"]) / med(t["plain"]), "streamed_bytes": stream_bytes,
           "window_bytes_per_s": stream_bytes / (med(t["window"]) * 1e-3),
           "extract_min1_ms": med(t["extract1"]), "extract_min10_ms": med(t["extract10"]), "extract_min1_entries": entries[1],
           "extract_min10_entries": entries[10], "windows_per_feed": windows_per_feed, "feeds": feeds, "last_minus_pos_max": span_max,
           "entries_ascending": ascending, "counts_divisible_by_feeds": divisible,
           "sample_reads": k, "sample_entries": len(want), "sample_identical": bool(sample_ok),
           "plain_ms_all": t["plain"], "pair_ms_all": t["pair"], "window_ms_all": t["window"], "composed_ms_all": t["composed"],
           "extract_min1_ms_all": t["extract1"], "extract_min10_ms_all": t["extract10"]}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ok = n_pairs == pairs.n_pairs and ascending and divisible and sample_ok and entries[1] == fed
    epi.close()
    pairs.close()
    idx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
