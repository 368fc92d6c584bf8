#!/usr/bin/env python3
"""Cost of the two passes behind bin/walt -MS (include/walt_amd.h, "called sites") beside their two siblings on the same
resident counters, on the hg19-like genome: one process, one batch of C->T reads (tools/synth.py's make_reads: 5 % of the
C's stay, in every context) mapped and piled up once, and a second batch drawn from one stretch of --hot-mbp Mbp alone, so
that the library also has sites of depth 32 and more (the histogram's global atomics), sites deeper than 127 (the deep
path) and sites that pass the test (records for the calls pass to store); then over the whole genome on one stream,
alternating, timed by device events after a warm-up:
  hist     walt_pileup_depth_hist_device: the joint histogram of (depth, meth) per context
  levels   walt_pileup_levels_device: the genome-wide summary, the heavier sibling
  count    walt_pileup_extract_device with cap 0 (k_pile_count and the scan): the floor of a pass over these bytes
  empty    the histogram pass over a second pile-up of the same index that holds no call: the walk without any site
  calls    walt_pileup_call_sites_device with the table Benjamini-Hochberg gives at --rate and --alpha (count, scan, write)
and, on the host, Benjamini-Hochberg over the four contexts' histograms and the deep sites (sitecall_core.h, compiled here
with g++ through tests/sitecall_harness.cpp).  No rate is fixed in advance: the tool reports the times, where the
histogram lands between the count and the summary, the counter bytes per second of each, the share of deep sites, and
checks the histogram and the called sites of one window against numpy folds of the extraction (tests/test_gpu_sitecall.py).
Prints one JSON line.

  python3 tools/sitecall_bench.py [--reads 20000000] [--read-len 100] [--steps 10] [--warmup 2] [--window 200000]
                                  [--rate 0.005] [--alpha 0.01] [--hot-mbp 5] [--hot-reads 10000000] [--genome-mbp <size>]
                                  [--out profiles/sitecall_hg19like.json]"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

STREAM_RATE = 6.3e12       # bytes/s a streaming kernel can reach on the device (tools/meth_bench.py)


def log(msg):
    print("[sitecall_bench] " + msg, file=sys.stderr, flush=True)


def host_harness(tmp):
    """sitecall_core.h's host half as a library (the one tests/test_sitecall_cpu.py builds)"""
    so = os.path.join(tmp, "libsitecall_harness.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fopenmp", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "walt_amd", "csrc"),
                    os.path.join(ROOT, "tests", "sitecall_harness.cpp"), "-o", so], check=True, timeout=300)
    L = ctypes.CDLL(so)
    vp = ctypes.c_void_p
    L.sitecall_harness_context.argtypes = [vp, vp, vp, ctypes.c_uint64, ctypes.c_double, ctypes.c_double, ctypes.c_uint32, vp, vp, vp]
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--read-len", type=int, default=100)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--genome-mbp", type=float, default=None, help="synthetic genome size (default: full scale)")
    ap.add_argument("--window", type=int, default=200_000, help="positions whose histogram and calls the folds check")
    ap.add_argument("--rate", type=float, default=0.005, help="the non-conversion rate of the test")
    ap.add_argument("--alpha", type=float, default=0.01, help="the false discovery rate")
    ap.add_argument("--hot-mbp", type=float, default=5.0, help="the stretch the second batch is drawn from (0: no second batch)")
    ap.add_argument("--hot-reads", type=int, default=10_000_000, help="reads of the second batch (at most --reads)")
    ap.add_argument("--max-mismatches", type=int, default=6)
    ap.add_argument("--bucket", type=int, default=5000)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()

    import torch
    import synth
    import walt_amd
    import test_gpu_sitecall as rule_of
    tmp = tempfile.mkdtemp(prefix="sitecall_bench_")
    H = host_harness(tmp)
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
    torch.cuda.empty_cache()
    t0 = time.perf_counter()
    idx = walt_amd.Index.build_device(genome_ascii.data_ptr(), lens, names, device=0, strands=walt_amd.STRANDS_ALL)
    idx.enable_reference()
    torch.cuda.synchronize()
    log("index (4 strands) + reference: %.1f GB in HBM (%.1f s)" % (idx.device_bytes / 1e9, time.perf_counter() - t0))
    n, L = args.reads, args.read_len
    d_bases, _ = synth.make_reads(torch, dev, genome_ascii, n, L, seed=1000, ag=False)
    # the second batch: reads of one stretch inside the largest sequence, a tenth of the way in
    n_hot = min(args.hot_reads, n) if args.hot_mbp > 0 else 0
    big = int(np.argmax(lens))
    hot_len = min(int(args.hot_mbp * 1e6), int(lens[big]) // 2)
    h_lo = int(start[big]) + int(lens[big]) // 10
    d_hot = synth.make_reads(torch, dev, genome_ascii[h_lo:h_lo + hot_len], n_hot, L, seed=1001, ag=False)[0] if n_hot else None
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
    if n_hot:
        t0 = time.perf_counter()
        idx.map_se_batch_device(d_hot.data_ptr(), d_off.data_ptr(), n_hot, L, d_recs.data_ptr(), d_stats.data_ptr(), d_ws.data_ptr(), ws,
                                stream=stream, ag_wildcard=False, max_mismatches=args.max_mismatches, b=args.bucket)
        pile.add_batch_device(d_hot.data_ptr(), d_off.data_ptr(), n_hot, d_recs.data_ptr(), 16, None, 1, "T", stream=stream)
        torch.cuda.synchronize()
        walt_amd.Index.check_batch(d_ws.data_ptr(), stream)
        log("a second batch of %d reads from [%d, %d) mapped and piled up (%.1f s)" % (n_hot, h_lo, h_lo + hot_len, time.perf_counter() - t0))
    del d_ws, d_bases, d_off, d_recs, d_hot
    torch.cuda.empty_cache()

    # the histogram once, Benjamini-Hochberg on the host, and the table the calls pass takes
    hist, deep = pile.depth_hist()
    n_sites = int(hist.sum() + deep.sum())
    none = np.tile(np.arange(1, 129, dtype=np.uint32), (4, 1))
    deep_sites = pile.call_sites(none) if int(deep.sum()) <= 50_000_000 else None  # (a library this deep is not what this is for)
    table = np.zeros((4, 128), dtype=np.uint32)
    bh = []
    t_bh = []
    for rep in range(3):
        t0 = time.perf_counter()
        bh = []
        for c in range(4):
            mine = deep_sites[deep_sites["context"] == c] if deep_sites is not None else np.zeros(0, dtype=walt_amd.meth_site_dtype)
            dd = (mine["meth"].astype(np.uint64) + mine["unmeth"].astype(np.uint64)).copy()
            dm = mine["meth"].astype(np.uint64).copy()
            out = np.zeros(2, dtype=np.uint64)
            cutoff = ctypes.c_double(0.0)
            row = np.zeros(128, dtype=np.uint32)
            has = H.sitecall_harness_context(hist[c].ctypes.data, dd.ctypes.data, dm.ctypes.data, len(mine), args.rate, args.alpha, 1,
                                             row.ctypes.data, out.ctypes.data, ctypes.byref(cutoff))
            table[c] = row
            bh.append({"tested": int(out[0]), "called": int(out[1]), "cutoff": cutoff.value if has else None,
                       "occupied_bins": int((hist[c] != 0).sum()), "deep": int(deep[c])})
        t_bh.append((time.perf_counter() - t0) * 1e3)
    log("host: Benjamini-Hochberg over four contexts in %.2f ms; %s" % (min(t_bh), bh))

    dev_bytes = 8 * 4 * walt_amd.SITECALL_BINS
    d_hist = torch.zeros(4 * walt_amd.SITECALL_BINS, dtype=torch.int64, device=dev)
    d_deep = torch.zeros(4, dtype=torch.int64, device=dev)
    d_lv = torch.zeros(82, dtype=torch.int64, device=dev)
    d_n = torch.zeros(3, dtype=torch.int64, device=dev)
    d_table = torch.from_numpy(table.view(np.int32)).to(dev)
    cap = sum(b["called"] for b in bh) + int(deep.sum()) + 1
    d_out = torch.zeros((cap, 2), dtype=torch.int64, device=dev)
    d_nc = torch.zeros(1, dtype=torch.int64, device=dev)

    bare = idx.pileup()  # no call: the walk of the histogram pass without a site

    def walk():
        bare.depth_hist_device(0, glen, d_hist.data_ptr(), d_deep.data_ptr(), stream=stream)

    def histogram():
        pile.depth_hist_device(0, glen, d_hist.data_ptr(), d_deep.data_ptr(), stream=stream)

    def summary():
        pile.levels_device(0, glen, d_lv.data_ptr(), stream=stream)

    def counting():
        pile.extract_device(0, glen, None, 0, d_n.data_ptr(), d_n.data_ptr() + 8, stream=stream)

    def calling():
        pile.call_sites_device(0, glen, d_table.data_ptr(), d_out.data_ptr(), cap, d_nc.data_ptr(), stream=stream)

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    legs = (("empty", walk), ("hist", histogram), ("levels", summary), ("count", counting), ("calls", calling))
    for _ in range(args.warmup):
        for _, fn in legs:
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k, _ in legs}
    for _ in range(args.steps):  # alternating, so that clock and temperature drift hit every leg alike
        for k, fn in legs:
            t[k].append(once(fn))
    med = {k: float(np.median(v)) for k, v in t.items()}
    n_count = int(d_n.cpu().numpy()[0])
    n_called = int(d_nc.item())
    same_hist = d_hist.cpu().numpy().tobytes() == hist.tobytes() and d_deep.cpu().numpy().tobytes() == deep.tobytes()
    want_called = int(deep.sum()) + sum(int(hist[c, rule_of.site_bin(d, int(table[c, d])):rule_of.site_bin(d, d) + 1].sum())
                                        for c in range(4) for d in range(1, 128) if table[c, d] <= d)
    consistent = same_hist and n_count == n_sites and n_called == want_called
    log("medians of %d, ms: %s; %d sites (the count pass: %d), %d deep, %d called" % (args.steps, med, n_sites, n_count, int(deep.sum()), n_called))

    # exactness: the window's histogram and calls against numpy folds of its extraction
    sites, _ = pile.extract(w_lo, w_hi)
    wh, wd = pile.depth_hist(w_lo, w_hi)
    fh, fd = rule_of.fold_sites(sites)
    identical = bool(np.array_equal(wh, fh) and np.array_equal(wd, fd) and
                     pile.call_sites(table, w_lo, w_hi).tobytes() == rule_of.filter_sites(sites, table).tobytes())
    log("folds over [%d, %d): %d sites, %d chromosome starts inside: %s" % (
        w_lo, w_hi, len(sites), int(((start > w_lo) & (start < w_hi)).sum()), "identical" if identical else "DIFFERENT"))
    pile.close()
    bare.close()
    idx.close()
    counter_bytes = 8 * glen
    between = (med["hist"] - med["count"]) / (med["levels"] - med["count"]) if med["levels"] != med["count"] else None
    line = json.dumps({
        "tool": "sitecall_bench", "reads": n, "read_len": L, "genome_bp": glen, "steps": args.steps, "warmup": args.warmup,
        "rate": args.rate, "alpha": args.alpha, "counter_bytes": counter_bytes, "hist_bytes": dev_bytes,
        "hot": [h_lo, h_lo + hot_len, n_hot], "hist_empty_ms": med["empty"],
        "hist_ms": med["hist"], "levels_ms": med["levels"], "count_ms": med["count"], "calls_ms": med["calls"], "bh_host_ms": min(t_bh),
        "hist_between_count_and_levels": between,
        "hist_bytes_per_s": counter_bytes / (med["hist"] * 1e-3), "count_bytes_per_s": counter_bytes / (med["count"] * 1e-3),
        "hist_share_of_achievable": counter_bytes / (med["hist"] * 1e-3) / STREAM_RATE, "achievable_bytes_per_s": STREAM_RATE,
        "ms_all": t, "sites": n_sites, "deep_sites": int(deep.sum()), "deep_share": float(deep.sum()) / max(1, n_sites),
        "sites_above_lds_depth": int(hist[:, rule_of.site_bin(rule_of.LDS_DEPTH + 1, 0):].sum()),
        "sites_with_a_methylated_call": n_sites - int(sum(hist[:, rule_of.site_bin(d, 0)].sum() for d in range(1, 128))) - int(
            0 if deep_sites is None else (deep_sites["meth"] == 0).sum()),
        "contexts": bh, "called": n_called, "agree": consistent, "window": [w_lo, w_hi], "window_identical": identical,
    })
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if identical and consistent else 1


if __name__ == "__main__":
    sys.exit(main())
