#!/usr/bin/env python3
"""Cost of the genome-wide methylation summary (walt_pileup_levels_device) beside the count-only extraction
(walt_pileup_extract_device with cap 0: k_pile_count and the scan), which streams the same two counter planes and is the
yardstick, on the hg19-like genome: one process, one batch of C->T reads (tools/synth.py's make_reads) mapped and piled
up once, then both passes over the whole genome on one stream, alternating, timed by device events after a warm-up.
No rate is fixed in advance: the tool reports both times, their ratio and the counter bytes per second of each
(8 x genome_len bytes per pass) beside the achievable streaming rate.  The summary of one window is checked against the
restatement in tests/test_gpu_levels.py, from the counters Pileup.read returns and the genome's own bases (the
synthetic genome has no N, so they are the '+' reference).  Prints one JSON line.

  python3 tools/levels_bench.py [--reads 20000000] [--read-len 100] [--steps 10] [--warmup 2] [--window 200000]
                                [--genome-mbp <size>] [--out profiles/levels_hg19like.json]"""
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


def log(msg):
    print("[levels_bench] " + msg, file=sys.stderr, flush=True)


class Shifted:
    """a window of the genome's bases indexed by genome position"""

    def __init__(self, arr, lo):
        self.arr, self.lo = arr, lo

    def __getitem__(self, f):
        return self.arr[f - self.lo]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--read-len", type=int, default=100)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--genome-mbp", type=float, default=None, help="synthetic genome size (default: full scale)")
    ap.add_argument("--window", type=int, default=200_000, help="positions whose summary the restatement checks")
    ap.add_argument("--max-mismatches", type=int, default=6)
    ap.add_argument("--bucket", type=int, default=5000)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()

    import torch
    import synth
    import walt_amd
    import test_gpu_levels as rule_of
    from test_gpu_pileup import chrom_of, site_class
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    scale = 1.0 if args.genome_mbp is None else args.genome_mbp * 1e6 / synth.HG19_TOTAL
    t0 = time.perf_counter()
    genome_ascii, lens, names = synth.make_genome(torch, dev, scale, seed=2, kind="hg19like")
    torch.cuda.synchronize()
    glen = int(sum(lens))
    log("genome: %d bp in %d sequences (%.1f s)" % (glen, len(lens), time.perf_counter() - t0))
    start = np.zeros(len(lens) + 1, dtype=np.int64)
    start[1:] = np.cumsum(lens, dtype=np.int64)
    # the window: around the first chromosome boundary at or beyond a third of the genome, so that it holds one
    c_mid = min(len(lens) - 1, int(np.searchsorted(start, glen // 3, side="left")))
    w_lo = max(0, int(start[c_mid]) - args.window // 2)
    w_hi = min(glen, w_lo + args.window)
    r_lo, r_hi = max(0, w_lo - 2), min(glen, w_hi + 2)
    window_bases = genome_ascii[r_lo:r_hi].cpu().numpy()
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
    pile = idx.pileup()
    d_recs = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    d_stats = torch.zeros(4, dtype=torch.int64, device=dev)
    ws = walt_amd.lib().walt_se_workspace_bytes(n, L)
    d_ws = torch.empty(ws, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    t0 = time.perf_counter()
    idx.map_se_batch_device(d_bases.data_ptr(), d_off.data_ptr(), n, L, d_recs.data_ptr(), d_stats.data_ptr(), d_ws.data_ptr(), ws,
                            stream=stream, ag_wildcard=False, max_mismatches=args.max_mismatches, b=args.bucket)
    pile.add_batch_device(d_bases.data_ptr(), d_off.data_ptr(), n, d_recs.data_ptr(), 16, None, 1, "T", stream=stream)
    torch.cuda.synchronize()
    walt_amd.Index.check_batch(d_ws.data_ptr(), stream)
    log("one batch of %d reads mapped and piled up (%.1f s)" % (n, time.perf_counter() - t0))
    del d_ws, d_bases, d_off, d_recs
    torch.cuda.empty_cache()

    d_lv = torch.zeros(82, dtype=torch.int64, device=dev)
    d_n = torch.zeros(3, dtype=torch.int64, device=dev)

    def summary():
        pile.levels_device(0, glen, d_lv.data_ptr(), stream=stream)

    def counting():
        pile.extract_device(0, glen, None, 0, d_n.data_ptr(), d_n.data_ptr() + 8, stream=stream)

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(args.warmup):
        summary()
        counting()
    torch.cuda.synchronize()
    t = {"levels": [], "count": []}
    for _ in range(args.steps):  # alternating, so that clock and temperature drift hit both legs alike
        t["levels"].append(once(summary))
        t["count"].append(once(counting))
    med = {k: float(np.median(v)) for k, v in t.items()}
    lv = rule_of.as_dict(d_lv.cpu().numpy().view(walt_amd.levels_dtype)[0])
    n_sites, off_m, off_u = (int(x) for x in d_n.cpu().numpy())
    covered = sum(lv["row"][r]["covered"] for r in range(4))
    log("medians of %d, ms: %s; %d covered sites (the count pass: %d)" % (args.steps, med, covered, n_sites))
    consistent = covered == n_sites and lv["offref"] == [off_m, off_u]

    # exactness: the summary of the window against the restatement
    R0 = Shifted(window_bases, r_lo)
    cls, pair = [], []
    for f in range(w_lo, w_hi):
        c = site_class(R0, start, f)
        cls.append(None if c is None else c[1])
        hi = chrom_of(start, f)[2]
        pair.append(chr(R0[f]) == "C" and f + 1 < hi and chr(R0[f + 1]) == "G")
    m, u = pile.read(w_lo, min(glen, w_hi + 1))
    want = rule_of.expected_levels(cls + [None], pair + [False], np.append(m, 0), np.append(u, 0), 0, w_hi - w_lo)
    got = rule_of.as_dict(pile.levels(w_lo, w_hi))
    identical = got == want
    log("restatement over [%d, %d): %d sites, %d pairs, %d chromosome starts inside: %s" % (
        w_lo, w_hi, sum(want["row"][r]["sites"] for r in range(4)), want["row"][4]["sites"],
        int(((start > w_lo) & (start < w_hi)).sum()), "identical" if identical else "DIFFERENT"))
    pile.close()
    idx.close()
    counter_bytes = 8 * glen
    line = json.dumps({
        "tool": "levels_bench", "reads": n, "read_len": L, "genome_bp": glen, "steps": args.steps, "warmup": args.warmup,
        "counter_bytes": counter_bytes, "levels_ms": med["levels"], "count_ms": med["count"],
        "levels_over_count": med["levels"] / med["count"],
        "levels_bytes_per_s": counter_bytes / (med["levels"] * 1e-3), "count_bytes_per_s": counter_bytes / (med["count"] * 1e-3),
        "levels_share_of_achievable": counter_bytes / (med["levels"] * 1e-3) / STREAM_RATE,
        "count_share_of_achievable": counter_bytes / (med["count"] * 1e-3) / STREAM_RATE,
        "achievable_bytes_per_s": STREAM_RATE, "ms_all": t, "levels": lv, "count_sites": n_sites, "offref": [off_m, off_u],
        "levels_agree_with_count": consistent, "window": [w_lo, w_hi], "window_identical": identical,
    })
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if identical and consistent else 1


if __name__ == "__main__":
    sys.exit(main())
