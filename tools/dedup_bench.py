#!/usr/bin/env python3
"""Cost of duplicate marking (walt_dedup_batch_device) beside the mapping call it follows, on the hg19-like genome: one
process, one resident batch of C->T reads (tools/synth.py's make_reads; --dup-fraction of them copies of earlier reads
of the batch), timed on the same batch and stream, alternating, by device events after a warm-up:
  * the mapping call alone                   (walt_map_se_batch_device)
  * insert + mark on its records             (walt_dedup_batch_device on a cleared, reserved set)
  * a doubling                               (walt_dedup_reserve from the smallest table that holds the batch to twice that;
                                              wall time: the call is synchronous)
The verdicts of a prefix of the batch are checked against the restatement in tests/test_dedup_cpu.py.  The kernels' own
times come from running this tool under
    rocprofv3 --kernel-trace --stats -d <dir> -- python3 tools/dedup_bench.py ...
(k_dedup_insert, k_dedup_mark, k_dedup_rehash).  Prints one JSON line; --out also writes it to a file
(profiles/dedup_hg19like.json).

  python3 tools/dedup_bench.py [--reads 50000000] [--read-len 100] [--steps 10] [--warmup 2] [--dup-fraction 0.3]"""
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
    print("[dedup_bench] " + msg, file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=50_000_000)
    ap.add_argument("--read-len", type=int, default=100)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dup-fraction", type=float, default=0.3)
    ap.add_argument("--genome-mbp", type=float, default=None, help="synthetic genome size (default: full scale)")
    ap.add_argument("--check", type=int, default=200_000, help="records of the batch whose verdicts the restatement checks")
    ap.add_argument("--max-mismatches", type=int, default=6)
    ap.add_argument("--bucket", type=int, default=5000)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()

    import torch
    import synth
    import walt_amd
    import test_dedup_cpu as rule_of
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    scale = 1.0 if args.genome_mbp is None else args.genome_mbp * 1e6 / synth.HG19_TOTAL
    t0 = time.perf_counter()
    genome_ascii, lens, names = synth.make_genome(torch, dev, scale, seed=2, kind="hg19like")
    torch.cuda.synchronize()
    log("genome: %d bp in %d sequences (%.1f s)" % (int(sum(lens)), len(lens), time.perf_counter() - t0))
    torch.cuda.empty_cache()
    idx = walt_amd.Index.build_device(genome_ascii.data_ptr(), lens, names, device=0, strands=walt_amd.STRANDS_CT)
    torch.cuda.synchronize()
    n, L = args.reads, args.read_len
    d_bases, _ = synth.make_reads(torch, dev, genome_ascii, n, L, seed=1000, ag=False)
    del genome_ascii
    # copies: read i of the last dup-fraction of the batch becomes a copy of a random earlier read
    n_copy = int(n * args.dup_fraction)
    if n_copy:
        g = torch.Generator(device=dev)
        g.manual_seed(7)
        src = torch.randint(0, n - n_copy, (n_copy,), device=dev, generator=g)
        rows = d_bases.view(n, L)
        rows[n - n_copy:] = rows[src]
        del src, rows
    d_off = torch.arange(n + 1, device=dev, dtype=torch.int64) * L
    d_out = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    d_stats = torch.zeros(4, dtype=torch.int64, device=dev)
    d_dup = torch.zeros(n, dtype=torch.uint8, device=dev)
    ws = walt_amd.lib().walt_se_workspace_bytes(n, L)
    d_ws = torch.empty(ws, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    dd = walt_amd.Dedup(device=0, initial_slots=2 * n)
    log("duplicate set: %.2f GB" % (dd.device_bytes / 1e9))

    def mapping():
        idx.map_se_batch_device(d_bases.data_ptr(), d_off.data_ptr(), n, L, d_out.data_ptr(), d_stats.data_ptr(),
                                d_ws.data_ptr(), ws, stream=stream, ag_wildcard=False, max_mismatches=args.max_mismatches,
                                b=args.bucket)

    def marking():
        dd.add_batch_device(d_out.data_ptr(), n, d_dup.data_ptr(), 16, None, 1, "T", 0, stream=stream)

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(args.warmup):
        mapping()
        dd.clear()
        marking()
    torch.cuda.synchronize()
    walt_amd.Index.check_batch(d_ws.data_ptr(), stream)
    t = {"map": [], "dedup": []}
    for _ in range(args.steps):  # alternating, so that clock and temperature drift hit both legs alike
        t["map"].append(once(mapping))
        dd.clear()
        t["dedup"].append(once(marking))
    keys, fed = dd.count()
    dup = d_dup.cpu().numpy()
    k = min(args.check, n)
    recs = d_out[:16 * k].cpu().numpy().view(walt_amd.best_match_dtype)
    want = rule_of.expect_single(rule_of.DupRule(), recs, "T")
    assert dup[:k].tolist() == want.tolist(), "verdicts differ from the restatement"
    # a doubling: from the smallest table that holds what the set holds now to twice that
    t_double = []
    for _ in range(max(1, args.steps // 3)):
        small = walt_amd.Dedup(device=0, initial_slots=2 * n)
        small.add_batch_device(d_out.data_ptr(), n, d_dup.data_ptr(), 16, None, 1, "T", 0, stream=stream)
        k0, _ = small.count()
        before = small.device_bytes
        t0 = time.perf_counter()
        small.reserve(before // 32 + 1 - k0)  # one key more than half of the slots
        t_double.append((time.perf_counter() - t0) * 1e3)
        assert small.device_bytes > before
        small.close()
    med = lambda v: float(np.median(v))
    res = {"tool": "dedup_bench", "reads": n, "read_len": L, "dup_fraction": args.dup_fraction, "steps": args.steps,
           "map_ms": med(t["map"]), "dedup_ms": med(t["dedup"]), "dedup_over_map": med(t["dedup"]) / med(t["map"]),
           "records_per_s": n / (med(t["dedup"]) * 1e-3), "keys": keys, "fed_last_step": fed, "duplicates": int(dup.sum()),
           "doubling_ms": med(t_double), "set_bytes": dd.device_bytes, "checked_records": k}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    dd.close()
    idx.close()


if __name__ == "__main__":
    main()
