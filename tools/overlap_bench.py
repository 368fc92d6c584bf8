#!/usr/bin/env python3
"""Cost of the overlap of a pair (walt_pair_overlap_batch_device, walt_meth_pileup_batch_excl_device) beside the paired-end
mapping call it follows, on the hg19-like genome: one process, one resident batch of pairs (tools/synth.py's
make_pairs), timed on the same batch and stream, alternating, by device events after a warm-up:
  * the mapping call alone                         (walt_map_pe_batch_device)
  * the overlap kernel on its records              (walt_pair_overlap_batch_device, with totals)
  * mate 2's calls into a pile-up without excl     (walt_meth_pileup_batch_device)
  * the same with excl                             (walt_meth_pileup_batch_excl_device)
The interval words of a prefix of the batch are checked against the brute-force restatement in
tests/test_gpu_overlap.py.  The kernels' own times come from running this tool under
    rocprofv3 --kernel-trace --stats -d <dir> -- python3 tools/overlap_bench.py ...
(k_pair_overlap, k_meth_pile).  Prints one JSON line; --out also writes it to a file (profiles/overlap_hg19like.json).

  python3 tools/overlap_bench.py [--pairs 50000000] [--read-len 100] [--steps 10] [--warmup 2]"""
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
    print("[overlap_bench] " + msg, file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=50_000_000)
    ap.add_argument("--read-len", type=int, default=100)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--genome-mbp", type=float, default=None, help="synthetic genome size (default: full scale)")
    ap.add_argument("--check", type=int, default=20_000, help="pairs of the batch whose intervals the restatement checks")
    ap.add_argument("--max-mismatches", type=int, default=6)
    ap.add_argument("--bucket", type=int, default=5000)
    ap.add_argument("--top-k", type=int, default=50)
    ap.add_argument("--frag-range", type=int, default=1000)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()

    import torch
    import synth
    import walt_amd
    import test_gpu_overlap as rule_of
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
    mm, b, k, fr = args.max_mismatches, args.bucket, args.top_k, args.frag_range
    d_out = torch.zeros(n * 64, dtype=torch.uint8, device=dev)
    d_stats = torch.zeros(8, dtype=torch.int64, device=dev)
    d_excl = torch.zeros(n, dtype=torch.int32, device=dev)
    d_tot = torch.zeros(2, dtype=torch.int64, device=dev)
    ws = idx.pe_workspace_bytes(n, L, k)
    d_ws = torch.empty(ws, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    pile = idx.pileup()

    def mapping():
        idx.map_pe_batch_device(d1.data_ptr(), d_off.data_ptr(), d2.data_ptr(), d_off.data_ptr(), n, L, d_out.data_ptr(),
                                d_stats.data_ptr(), d_ws.data_ptr(), ws, stream=stream, max_mismatches=mm, b=b, top_k=k,
                                frag_range=fr)

    def overlap():
        idx.pair_overlap_device(d_out.data_ptr(), d_off.data_ptr(), d_off.data_ptr(), n, d_excl.data_ptr(), None, None,
                                d_tot.data_ptr(), stream=stream)

    def calls(with_excl):
        pile.add_batch_device(d2.data_ptr(), d_off.data_ptr(), n, d_out.data_ptr() + 16, 64, None, 1, "A", stream=stream,
                              d_excl=d_excl.data_ptr() if with_excl else None)

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(args.warmup):
        mapping()
        overlap()
        calls(False)
        calls(True)
    torch.cuda.synchronize()
    walt_amd.Index.check_batch(d_ws.data_ptr(), stream)
    t = {"map": [], "overlap": [], "calls": [], "calls_excl": []}
    for _ in range(args.steps):  # alternating, so that clock and temperature drift hit all legs alike
        t["map"].append(once(mapping))
        d_tot.zero_()
        t["overlap"].append(once(overlap))
        t["calls"].append(once(lambda: calls(False)))
        t["calls_excl"].append(once(lambda: calls(True)))
    totals = d_tot.cpu().numpy().tolist()
    m = min(args.check, n)
    got = d_excl[:m].cpu().numpy().view(np.uint32)
    res = d_out[:64 * m].cpu().numpy().view(walt_amd.pair_result_dtype)
    start = np.zeros(len(lens) + 1, dtype=np.uint32)
    start[1:] = np.cumsum(lens, dtype=np.uint64).astype(np.uint32)
    glen = int(sum(lens))
    want = [rule_of.word_of(rule_of.excluded_positions(start, glen, res["m1"][i], res["m2"][i], res["best_times"][i], L, L)[0])
            for i in range(m)]
    assert got.tolist() == want, "interval words differ from the restatement"
    med = lambda v: float(np.median(v))
    out = {"tool": "overlap_bench", "pairs": n, "read_len": L, "genome_bp": glen, "steps": args.steps, "warmup": args.warmup,
           "map_ms": med(t["map"]), "overlap_ms": med(t["overlap"]), "calls_ms": med(t["calls"]),
           "calls_excl_ms": med(t["calls_excl"]), "overlap_over_map": med(t["overlap"]) / med(t["map"]),
           "excl_over_plain_calls": med(t["calls_excl"]) / med(t["calls"]),
           "overlap_bytes_per_s": n * 110 / (med(t["overlap"]) * 1e-3), "pairs_with_interval": int(totals[0]),
           "bases_excluded": int(totals[1]), "unique_pairs": int((d_out.view(torch.int32).view(n, 16)[:, 8] == 1).sum()),
           "map_ms_all": t["map"], "overlap_ms_all": t["overlap"], "calls_ms_all": t["calls"], "calls_excl_ms_all": t["calls_excl"],
           "checked_pairs": m}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    pile.close()
    idx.close()


if __name__ == "__main__":
    main()
