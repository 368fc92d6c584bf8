#!/usr/bin/env python3
"""Cost of the base qualities (walt_meth_pileup_batch_qual_device) on the hg19-like genome: one process, one resident batch
of C->T reads (tools/synth.py's make_reads) mapped once, every leg timed on the same batch and stream, alternating, by
device events after a warm-up:
  * the calling call with the pile-up                  (walt_meth_pileup_batch_device: the parent commit's call)
  * the same with qualities at a floor of 0            (every base passes: the cost of the quality stream alone)
  * the same at Phred 20 over qualities drawn like the golden files' (uniform over '#' .. 'I', Phred 2 .. 40)
  * the evidence kernel without and with qualities at Phred 20.
The new legs are reported as ratios to the plain call of the same process, beside the ratio the added byte per base
predicts from the bytes the calling kernel moves (tools/meth_bench.py's account: the read, the calls written, the
record, the offsets and the reference words of a read; the pile-up's atomics are left out, so the prediction is an upper
bound of the ratio).  No time or ratio is fixed in advance.  The calls of a sample of reads at Phred 20 are checked against
the plain calls with '.' where the quality is below the floor.  Prints one JSON line and writes it to
profiles/qual_hg19like.json (--out).

  python3 tools/qual_bench.py [--reads 50000000] [--read-len 100] [--steps 10] [--warmup 2] [--genome-mbp N]"""
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
    print("[qual_bench] " + msg, file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=50_000_000)
    ap.add_argument("--read-len", type=int, default=100)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--genome-mbp", type=float, default=None, help="synthetic genome size (default: full scale)")
    ap.add_argument("--min-qual", type=int, default=20, help="the Phred floor of the third leg (offset 33)")
    ap.add_argument("--sample", type=int, default=200_000, help="reads whose calls are checked against the plain calls")
    ap.add_argument("--parent-spread", type=float, default=None,
                    help="the parent build's run-to-run spread of this session in per cent (tools/ab.sh), recorded beside the ratios")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qual_hg19like.json"))
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
    gen = torch.Generator(device=dev)
    gen.manual_seed(33)
    d_quals = torch.randint(35, 74, (n * L,), dtype=torch.uint8, device=dev, generator=gen)  # '#' .. 'I'
    floor = args.min_qual + 33
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
    out = (d_calls.data_ptr(), None, d_mstats.data_ptr())

    legs = {
        "plain": lambda: pile.add_batch_device(*batch, *out, stream=stream),
        "qual_floor_0": lambda: pile.add_batch_device(*batch, *out, stream=stream, quals=d_quals.data_ptr(), min_qual=0),
        "qual_floor": lambda: pile.add_batch_device(*batch, *out, stream=stream, quals=d_quals.data_ptr(), min_qual=floor),
        "evidence": lambda: ev.add_evidence_batch_device(*batch, stream=stream),
        "evidence_qual": lambda: ev.add_evidence_batch_device(*batch, stream=stream, quals=d_quals.data_ptr(), min_qual=floor),
    }

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
    for _ in range(args.steps):  # alternating, so that clock and temperature drift hit all legs alike
        for k, fn in legs.items():
            t[k].append(once(fn))
    med = {k: float(np.median(v)) for k, v in t.items()}
    spread = {k: 100.0 * (max(v) - min(v)) / float(np.median(v)) for k, v in t.items()}
    log("medians of %d, ms: %s" % (args.steps, med))

    # exactness: the calls of a sample at the floor are the plain calls with '.' where the quality is below it
    m = min(n, args.sample)
    legs["plain"]()
    torch.cuda.synchronize()
    plain = d_calls[:m * L].clone()
    d_mstats.zero_()
    legs["qual_floor"]()
    torch.cuda.synchronize()
    want = torch.where(d_quals[:m * L] >= floor, plain, torch.full_like(plain, ord(".")))
    identical = bool(torch.equal(d_calls[:m * L], want))
    letters = int((plain != ord(".")).sum())
    lost = int(((plain != ord(".")) & (want == ord("."))).sum())
    log("sample of %d reads: %s; %d of %d letters lost at Phred %d" % (m, "identical" if identical else "DIFFERENT", lost, letters, args.min_qual))
    pile.close()
    ev.close()
    idx.close()
    # bytes per read of the calling kernel without the pile-up's atomics: the bases, the calls, the record, two offsets, and
    # the reference words a read's slices gather (three words per 16-base slice, one slice more for the head)
    slices = (L + 15) // 16 + 1
    per_read = 2 * L + 16 + 16 + 12 * slices
    line = json.dumps({
        "tool": "qual_bench", "reads": n, "read_len": L, "genome_bp": glen, "steps": args.steps, "warmup": args.warmup,
        "min_qual": args.min_qual, "floor_byte": floor, "ms": med, "spread_percent": spread,
        "ratio_to_plain": {k: med[k] / med["plain"] for k in ("qual_floor_0", "qual_floor")},
        "ratio_evidence": med["evidence_qual"] / med["evidence"],
        "ratio_predicted_by_bytes": (per_read + L) / per_read, "bytes_per_read_plain": per_read, "bytes_per_read_added": L,
        "parent_spread_percent": args.parent_spread,
        "sample_reads": m, "sample_identical": identical, "sample_letters": letters, "sample_letters_lost": lost, "ms_all": t,
    })
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if identical else 1


if __name__ == "__main__":
    sys.exit(main())
