#!/usr/bin/env python3
"""Cost of ignored read ends (walt_meth_pileup_batch_trim_device, walt_pair_overlap_batch_trim_device) beside the calling
call without them, on the hg19-like genome: one process, one resident batch of pairs (tools/synth.py's make_pairs)
mapped once, then mate 2's calling call into a pile-up, with calls, counts and batch totals, timed on the same batch and
stream, alternating, by device events after a warm-up:
  * plain                  bounds (0, 0): the kernel a call always ran (k_meth_pile)
  * bounded                bounds (10, 10) (k_meth_pile_trim)
  * bounded with -NO       bounds (10, 10) and the interval of walt_pair_overlap_batch_trim_device (k_meth_pile_excl_trim)
The plain call's own spread over its repeated runs (minimum, median, maximum) is what the bounded legs are read against.
The calls of the first --check reads of each leg are compared with the restatement of tests/test_gpu_trim.py, the
intervals with its brute force.  Prints one JSON line; --out also writes it to a file (profiles/trim_hg19like.json).

  python3 tools/trim_bench.py [--pairs 20000000] [--read-len 100] [--steps 10] [--warmup 2] [--genome-mbp 1000]"""
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
    print("[trim_bench] " + msg, file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=20_000_000)
    ap.add_argument("--read-len", type=int, default=100)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--genome-mbp", type=float, default=None, help="synthetic genome size (default: full scale)")
    ap.add_argument("--check", type=int, default=20_000, help="reads of the batch whose calls the restatement checks")
    ap.add_argument("--trim5", type=int, default=10)
    ap.add_argument("--trim3", type=int, default=10)
    ap.add_argument("--max-mismatches", type=int, default=6)
    ap.add_argument("--bucket", type=int, default=5000)
    ap.add_argument("--top-k", type=int, default=50)
    ap.add_argument("--frag-range", type=int, default=1000)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()

    import torch
    import synth
    import walt_amd
    import test_gpu_trim as rule_of
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    scale = 1.0 if args.genome_mbp is None else args.genome_mbp * 1e6 / synth.HG19_TOTAL
    t0 = time.perf_counter()
    genome_ascii, lens, names = synth.make_genome(torch, dev, scale, seed=2, kind="hg19like")
    torch.cuda.synchronize()
    log("genome: %d bp in %d sequences (%.1f s)" % (int(sum(lens)), len(lens), time.perf_counter() - t0))
    torch.cuda.empty_cache()
    idx = walt_amd.Index.build_device(genome_ascii.data_ptr(), lens, names, device=0, strands=walt_amd.STRANDS_ALL)
    idx.enable_reference()
    n, L = args.pairs, args.read_len
    d1, d2, d_off = synth.make_pairs(torch, dev, genome_ascii, n, L, seed=2000 + L)
    del genome_ascii
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    d_out = torch.zeros(n * 64, dtype=torch.uint8, device=dev)
    d_stats = torch.zeros(8, dtype=torch.int64, device=dev)
    ws = idx.pe_workspace_bytes(n, L, args.top_k)
    d_ws = torch.empty(ws, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    idx.map_pe_batch_device(d1.data_ptr(), d_off.data_ptr(), d2.data_ptr(), d_off.data_ptr(), n, L, d_out.data_ptr(), d_stats.data_ptr(),
                            d_ws.data_ptr(), ws, stream=stream, max_mismatches=args.max_mismatches, b=args.bucket, top_k=args.top_k,
                            frag_range=args.frag_range)
    torch.cuda.synchronize()
    walt_amd.Index.check_batch(d_ws.data_ptr(), stream)
    del d_ws, d1
    torch.cuda.empty_cache()
    t1, t2 = (args.trim5, args.trim3), (args.trim5, args.trim3)  # both mates of the pair ignore the same ends
    d_excl = torch.zeros(n, dtype=torch.int32, device=dev)
    d_tot = torch.zeros(2, dtype=torch.int64, device=dev)
    idx.pair_overlap_device(d_out.data_ptr(), d_off.data_ptr(), d_off.data_ptr(), n, d_excl.data_ptr(), None, None, d_tot.data_ptr(),
                            stream=stream, trim1=t1, trim2=t2)
    d_calls = torch.zeros(n * L, dtype=torch.uint8, device=dev)
    d_counts = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    d_mstats = torch.zeros(9, dtype=torch.int64, device=dev)
    pile = idx.pileup()
    legs = {"plain": dict(), "bounded": dict(trim5=t2[0], trim3=t2[1]),
            "bounded_no_overlap": dict(trim5=t2[0], trim3=t2[1], d_excl=d_excl.data_ptr())}

    def call(leg):
        pile.add_batch_device(d2.data_ptr(), d_off.data_ptr(), n, d_out.data_ptr() + 16, 64, None, 1, "A", None, d_calls.data_ptr(),
                              d_counts.data_ptr(), d_mstats.data_ptr(), stream=stream, **legs[leg])

    def once(leg):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call(leg)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(args.warmup):
        for leg in legs:
            call(leg)
    torch.cuda.synchronize()
    t = {leg: [] for leg in legs}
    for _ in range(args.steps):  # alternating, so that clock and temperature drift hit all legs alike
        for leg in legs:
            t[leg].append(once(leg))
    # the restatement over the first reads of the batch, leg by leg
    m = min(args.check, n)
    res = d_out[:64 * m].cpu().numpy().view(walt_amd.pair_result_dtype)
    reads2 = [row.tobytes().decode() for row in d2.view(n, L)[:m].cpu().numpy()]
    got_words = d_excl[:m].cpu().numpy().view(np.uint32)
    got_calls = {}
    for leg in legs:
        call(leg)
        torch.cuda.synchronize()
        got_calls[leg] = d_calls[:m * L].cpu().numpy().tobytes().decode("latin-1")
    totals = d_tot.cpu().numpy().tolist()
    del d_calls, d_counts, d2
    torch.cuda.empty_cache()
    t0 = time.perf_counter()
    strands = [idx.export_strand(s)[0] for s in range(4)]
    R = [np.where(strands[2 + o] == ord("C"), np.uint8(ord("C")), strands[o]) for o in (0, 1)]
    del strands
    start = np.zeros(len(lens) + 1, dtype=np.int64)
    start[1:] = np.cumsum(lens, dtype=np.int64)
    glen = int(sum(lens))
    ex, words, _ = rule_of.want_words(start, glen, res, ["A" * L] * m, reads2, None, None, t1, t2)
    identical = {"intervals": bool(got_words.tolist() == words.tolist())}
    for leg, (trim, e) in (("plain", ((0, 0), None)), ("bounded", (t2, None)), ("bounded_no_overlap", (t2, ex))):
        want = rule_of.want_mate(R, start, reads2, res["m2"], "A", None, e, None, trim)
        identical[leg] = bool("".join(want[0]) == got_calls[leg])
    log("restatement over %d reads: %s (%.1f s)" % (m, identical, time.perf_counter() - t0))
    med = lambda v: float(np.median(v))
    plain = t["plain"]
    out = {"tool": "trim_bench", "pairs": n, "read_len": L, "genome_bp": glen, "steps": args.steps, "warmup": args.warmup,
           "trim5": args.trim5, "trim3": args.trim3,
           "plain_ms": med(plain), "plain_ms_min": min(plain), "plain_ms_max": max(plain), "plain_spread_ms": max(plain) - min(plain),
           "bounded_ms": med(t["bounded"]), "bounded_no_overlap_ms": med(t["bounded_no_overlap"]),
           "bounded_minus_plain_ms": med(t["bounded"]) - med(plain),
           "bounded_no_overlap_minus_plain_ms": med(t["bounded_no_overlap"]) - med(plain),
           "bounded_over_plain": med(t["bounded"]) / med(plain), "bounded_no_overlap_over_plain": med(t["bounded_no_overlap"]) / med(plain),
           "bounded_within_plain_spread": bool(med(t["bounded"]) - med(plain) <= max(plain) - min(plain)),
           "pairs_with_interval": int(totals[0]), "bases_excluded": int(totals[1]),
           "unique_pairs": int((d_out.view(torch.int32).view(n, 16)[:, 8] == 1).sum()),
           "checked_reads": m, "identical": identical,
           "plain_ms_all": plain, "bounded_ms_all": t["bounded"], "bounded_no_overlap_ms_all": t["bounded_no_overlap"]}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    pile.close()
    idx.close()
    return 0 if all(identical.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
