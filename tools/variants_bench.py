#!/usr/bin/env python3
"""Cost of the opposite-strand evidence (walt_meth_pileup_batch_ev_device, walt_meth_evidence_batch_device) and of the
two passes over it (walt_pileup_mask_variants_device, walt_pileup_variants_device) on the hg19-like genome: one process,
one resident batch of C->T reads (tools/synth.py's make_reads) mapped once, every leg timed on the same batch and stream,
alternating, by device events after a warm-up:
  * the calling call with the pile-up                 (walt_meth_pileup_batch_device: the parent commit's call)
  * the same plus the evidence                        (walt_meth_pileup_batch_ev_device)
  * the evidence kernel alone, under both add shapes  (option pile_rows 0 / 1)
  * the masking pass over the whole genome, beside walt_pileup_levels_device over the same range
  * the extraction of the flagged positions over the whole genome.
No time or ratio is fixed in advance.  The evidence of a window of the genome is checked against the restatement in
tests/test_gpu_variants.py, from the records of every read that reaches the window.  Prints one JSON line and writes it to
profiles/variants_hg19like.json (--out).

  python3 tools/variants_bench.py [--reads 50000000] [--read-len 100] [--steps 10] [--warmup 2] [--genome-mbp N]"""
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
    print("[variants_bench] " + msg, file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=50_000_000)
    ap.add_argument("--read-len", type=int, default=100)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--genome-mbp", type=float, default=None, help="synthetic genome size (default: full scale)")
    ap.add_argument("--window", type=int, default=500_000, help="positions whose evidence the restatement checks")
    ap.add_argument("--min-depth", type=int, default=5)
    ap.add_argument("--max-percent", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "variants_hg19like.json"))
    args = ap.parse_args()

    import torch
    import synth
    import walt_amd
    import test_gpu_variants as rule_of
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
    pile, ev = idx.pileup(), idx.pileup()
    d_out = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    d_stats = torch.zeros(4, dtype=torch.int64, device=dev)
    d_calls = torch.zeros(n * L, dtype=torch.uint8, device=dev)
    d_mstats = torch.zeros(9, dtype=torch.int64, device=dev)
    ws = walt_amd.lib().walt_se_workspace_bytes(n, L)
    d_ws = torch.empty(ws, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    idx.map_se_batch_device(d_bases.data_ptr(), d_off.data_ptr(), n, L, d_out.data_ptr(), d_stats.data_ptr(), d_ws.data_ptr(), ws,
                            stream=stream, ag_wildcard=False, max_mismatches=6, b=5000)
    walt_amd.Index.check_batch(d_ws.data_ptr(), stream)
    del d_ws
    torch.cuda.empty_cache()
    batch = (d_bases.data_ptr(), d_off.data_ptr(), n, d_out.data_ptr(), 16, None, 1, "T", None)

    def piling():
        pile.add_batch_device(*batch, d_calls.data_ptr(), None, d_mstats.data_ptr(), stream=stream)

    def piling_with_evidence():
        pile.add_batch_device(*batch, d_calls.data_ptr(), None, d_mstats.data_ptr(), stream=stream, evidence=ev)

    def evidence_alone():
        ev.add_evidence_batch_device(*batch, stream=stream)

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(args.warmup):
        piling()
        piling_with_evidence()
        evidence_alone()
    torch.cuda.synchronize()
    t = {k: [] for k in ("pile", "pile_ev", "ev_lane", "ev_rows")}
    for _ in range(args.steps):  # alternating, so that clock and temperature drift hit all legs alike
        idx.set_option("pile_rows", 0)
        t["pile"].append(once(piling))
        t["pile_ev"].append(once(piling_with_evidence))
        t["ev_lane"].append(once(evidence_alone))
        idx.set_option("pile_rows", 1)
        t["ev_rows"].append(once(evidence_alone))
        idx.set_option("pile_rows", 0)
    med = {k: float(np.median(v)) for k, v in t.items()}
    log("medians of %d, ms: %s" % (args.steps, med))

    # one known state for the passes: both objects cleared, then the batch once
    pile.clear()
    ev.clear()
    d_mstats.zero_()
    piling_with_evidence()
    torch.cuda.synchronize()
    calls = int(d_mstats.cpu().numpy()[1:9].sum())
    d_tot = torch.zeros(8, dtype=torch.int64, device=dev)
    d_lv = torch.zeros(82, dtype=torch.int64, device=dev)
    rule = (args.min_depth, args.max_percent)
    pile.variants_device(ev, 0, glen, *rule, None, 0, d_tot.data_ptr(), stream=stream)  # count alone
    torch.cuda.synchronize()
    n_flagged = int(d_tot[0])
    d_rows = torch.empty((n_flagged + 1, 24), dtype=torch.uint8, device=dev)

    def extracting():
        pile.variants_device(ev, 0, glen, *rule, d_rows.data_ptr(), n_flagged + 1, d_tot.data_ptr(), stream=stream)

    def masking():
        pile.mask_variants_device(ev, 0, glen, *rule, d_tot.data_ptr() + 8, stream=stream)

    def levels():
        pile.levels_device(0, glen, d_lv.data_ptr(), stream=stream)

    extracting()
    torch.cuda.synchronize()
    k = max(3, args.steps // 2)
    p = {"extract": [], "mask": [], "levels": []}
    totals = None
    for _ in range(k):
        p["extract"].append(once(extracting))
        p["levels"].append(once(levels))
        p["mask"].append(once(masking))  # (the first one removes the calls; the stream over R and the evidence is the same)
        totals = totals or [int(x) for x in d_tot.cpu().numpy()[1:6]]
    pmed = {k2: float(np.median(v)) for k2, v in p.items()}
    updates = 0  # the evidence of one feed, summed window by window
    for lo in range(0, glen, 1 << 26):
        m, o = ev.read(lo, min(glen, lo + (1 << 26)))
        updates += int(m.sum(dtype=np.int64)) + int(o.sum(dtype=np.int64))
    log("calls per feed %d, evidence updates per feed %d; %d flagged; passes, ms: %s" % (calls, updates, n_flagged, pmed))

    # exactness: the evidence of a window against the restatement, from the records of the reads that can reach it
    w_lo = glen // 3
    w_hi = min(glen, w_lo + args.window)
    rec = d_out.view(torch.int32).view(n, 4)
    pos = rec[:, 0].to(torch.int64) & 0xFFFFFFFF
    strands = [idx.export_strand(s)[0] for s in range(4)]
    R = [np.where(strands[2 + o] == ord("C"), np.uint8(ord("C")), strands[o]) for o in (0, 1)]
    del strands
    start = np.zeros(len(lens) + 1, dtype=np.int64)
    start[1:] = np.cumsum(lens, dtype=np.int64)
    c_lo = int(np.searchsorted(start, w_lo, side="right")) - 1
    c_hi = int(np.searchsorted(start, w_hi - 1, side="right")) - 1
    sel = (rec[:, 1] == 1) & (pos >= int(start[c_lo])) & (pos < int(start[c_hi + 1]))
    ids = torch.nonzero(sel).flatten()
    sub_recs = d_out.view(n, 16)[ids].cpu().numpy().reshape(-1).view(walt_amd.best_match_dtype)
    sub_bases = d_bases.view(n, L)[ids].cpu().numpy()
    q = sub_recs["genome_pos"].astype(np.int64)
    c = np.searchsorted(start, q, side="right") - 1
    a = np.where(sub_recs["strand"] == b"+", q, start[c] + start[c + 1] - q - L)
    keep = np.nonzero((a < w_hi) & (a + L > w_lo))[0]
    acc = (np.zeros(glen, dtype=np.uint16), np.zeros(glen, dtype=np.uint16))
    match, other = rule_of.expected_evidence(R, start, [sub_bases[i].tobytes() for i in keep], sub_recs[keep], "T", into=acc)
    gm, go = ev.read(w_lo, w_hi)
    identical = bool(np.array_equal(gm, match[w_lo:w_hi]) and np.array_equal(go, other[w_lo:w_hi]))
    log("restatement over [%d, %d): %d reads: %s" % (w_lo, w_hi, len(keep), "identical" if identical else "DIFFERENT"))
    pile.close()
    ev.close()
    idx.close()
    stream_bytes = 8.25 * glen  # R and the two evidence planes
    line = json.dumps({
        "tool": "variants_bench", "reads": n, "read_len": L, "genome_bp": glen, "steps": args.steps, "warmup": args.warmup,
        "rule": list(rule), "calling_with_pileup_ms": med["pile"], "calling_with_pileup_and_evidence_ms": med["pile_ev"],
        "evidence_added_ms": med["pile_ev"] - med["pile"],
        "evidence_alone_ms": {"lane_per_slice": med["ev_lane"], "neighbouring_lanes": med["ev_rows"]},
        "calls_per_feed": calls, "evidence_updates_per_feed": updates,
        "evidence_updates_per_s": {"lane_per_slice": updates / (med["ev_lane"] * 1e-3), "neighbouring_lanes": updates / (med["ev_rows"] * 1e-3)},
        "mask_ms": pmed["mask"], "levels_ms_same_range": pmed["levels"], "mask_stream_bytes_per_s": stream_bytes / (pmed["mask"] * 1e-3),
        "extract_ms": pmed["extract"], "flagged": n_flagged, "mask_totals": totals,
        "ms_all": t, "passes_ms_all": p, "window": [w_lo, w_hi], "window_reads": int(len(keep)), "window_identical": identical,
    })
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if identical else 1


if __name__ == "__main__":
    sys.exit(main())
