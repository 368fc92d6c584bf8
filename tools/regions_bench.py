#!/usr/bin/env python3
"""Cost of the per-region methylation summary (walt_pileup_regions_device) on the hg19-like genome: one process, one
batch of C->T reads (tools/synth.py's make_reads) mapped and piled up once, then three region sets on one stream, timed
by device events after a warm-up, in rounds that alternate with the yardstick:
  (a) 1,000-base tiles that partition the genome,
  (b) about 28,000 regions of 200 to 3,000 bases at random places (CpG islands in number and size),
  (c) 100-base tiles over the first 400 Mbp.
The yardstick is the genome-wide summary (walt_pileup_levels_device) over the same positions -- the whole genome for
(a), the first 400 Mbp for (c); (b) has none, its positions are reported.  No ratio is fixed in advance.  Two more
sets take (a)'s time apart: the genome as one region (the walk alone) and (a)'s number of empty regions (the memset and
the scan alone); what (a) takes beyond their sum is the search, the folds and the atomics per tile.  The records of
(a) must fold to the genome-wide summary in the fields they have, and a sample of (b) must equal the summaries of its
ranges; the tool exits non-zero otherwise.  Prints one JSON line.

  python3 tools/regions_bench.py [--reads 20000000] [--read-len 100] [--steps 10] [--warmup 2] [--genome-mbp <size>]
                                 [--out profiles/regions_hg19like.json]"""
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

FIELDS = ("sites", "covered", "meth", "unmeth", "level_sum")


def log(msg):
    print("[regions_bench] " + msg, file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--read-len", type=int, default=100)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
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
    glen = int(sum(lens))
    log("genome: %d bp in %d sequences (%.1f s)" % (glen, len(lens), time.perf_counter() - t0))
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

    # the region sets
    head = min(glen, 400_000_000)
    rng = np.random.RandomState(28)
    lo_a = np.arange(0, glen, 1000, dtype=np.int64)
    set_a = np.stack([lo_a, np.minimum(lo_a + 1000, glen)], axis=1)
    lo_b = rng.randint(0, glen - 3000, size=28000).astype(np.int64)
    set_b = np.stack([lo_b, lo_b + rng.randint(200, 3001, size=28000)], axis=1)
    lo_c = np.arange(0, head, 100, dtype=np.int64)
    set_c = np.stack([lo_c, np.minimum(lo_c + 100, head)], axis=1)
    # two more that take (a)'s time apart: the genome as one region (the walk alone: one search per run, a record
    # reached once per run) and as many empty regions as (a) has tiles (the memset and the scan alone: no unit)
    set_whole = np.array([[0, glen]], dtype=np.int64)
    set_empty = np.stack([lo_a, lo_a], axis=1)
    sets = {"a": set_a, "b": set_b, "c": set_c, "whole": set_whole, "empty": set_empty}
    assert all(len(s) <= walt_amd.REGIONS_MAX for s in sets.values())
    n_max = max(len(s) for s in sets.values())
    d_regs = {k: torch.from_numpy(s.astype(np.uint32).view(np.int32)).to(dev) for k, s in sets.items()}
    d_out = {k: torch.zeros(len(s) * 20, dtype=torch.int64, device=dev) for k, s in sets.items()}
    d_work = torch.empty(walt_amd.regions_workspace_bytes(n_max), dtype=torch.uint8, device=dev)
    d_lv = {k: torch.zeros(82, dtype=torch.int64, device=dev) for k in ("genome", "head")}

    def regions(k):
        return lambda: pile.regions_device(d_regs[k].data_ptr(), len(sets[k]), d_out[k].data_ptr(), d_work.data_ptr(), stream=stream)

    legs = {"regions_a": regions("a"), "regions_b": regions("b"), "regions_c": regions("c"),
            "regions_whole": regions("whole"), "regions_empty": regions("empty"),
            "levels_genome": lambda: pile.levels_device(0, glen, d_lv["genome"].data_ptr(), stream=stream),
            "levels_head": lambda: pile.levels_device(0, head, d_lv["head"].data_ptr(), stream=stream)}

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(args.warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in legs}
    for _ in range(args.steps):  # alternating, so that clock and temperature drift hit every leg alike
        for k, fn in legs.items():
            t[k].append(once(fn))
    med = {k: float(np.median(v)) for k, v in t.items()}
    log("medians of %d, ms: %s" % (args.steps, med))

    # exactness: set (a) folds to the genome-wide summary; a sample of (b) equals the summaries of its ranges
    lv = d_lv["genome"].cpu().numpy().view(walt_amd.levels_dtype)[0]
    rec_a = np.frombuffer(d_out["a"].cpu().numpy().tobytes(), dtype=walt_amd.region_levels_dtype)
    fold = {f: [int(rec_a["row"][f][:, r].astype(np.uint64).sum(dtype=np.uint64)) for r in range(5)] for f in FIELDS}
    want = {f: [int(lv["row"][r][f]) for r in range(5)] for f in FIELDS}
    folds = fold == want
    log("set (a): %d records fold to the genome-wide summary: %s" % (len(set_a), "yes" if folds else "NO"))
    rec_b = np.frombuffer(d_out["b"].cpu().numpy().tobytes(), dtype=walt_amd.region_levels_dtype)
    sample_ok = True
    for i in range(0, len(set_b), 700):
        one = pile.levels(int(set_b[i, 0]), int(set_b[i, 1]))
        sample_ok = sample_ok and all(int(rec_b[i]["row"][r][f]) == int(one["row"][r][f]) for r in range(5) for f in FIELDS)
    log("set (b): a sample of %d records equals the summaries of their ranges: %s" % (len(range(0, len(set_b), 700)), "yes" if sample_ok else "NO"))
    pile.close()
    idx.close()
    positions = {k: int((v[:, 1] - v[:, 0]).sum()) for k, v in sets.items()}
    line = json.dumps({
        "tool": "regions_bench", "reads": n, "read_len": L, "genome_bp": glen, "steps": args.steps, "warmup": args.warmup,
        "regions": {k: len(s) for k, s in sets.items()}, "positions": positions, "ms": med,
        "a_over_levels_genome": med["regions_a"] / med["levels_genome"], "c_over_levels_head": med["regions_c"] / med["levels_head"],
        "b_positions_per_s": positions["b"] / (med["regions_b"] * 1e-3), "a_positions_per_s": positions["a"] / (med["regions_a"] * 1e-3),
        "c_positions_per_s": positions["c"] / (med["regions_c"] * 1e-3), "ms_all": t,
        "a_minus_whole_minus_empty_ms": med["regions_a"] - med["regions_whole"] - med["regions_empty"],
        "a_folds_to_levels": folds, "b_sample_equals_levels": sample_ok,
    })
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if folds and sample_ok else 1


if __name__ == "__main__":
    sys.exit(main())
