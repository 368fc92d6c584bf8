#!/usr/bin/env python3
"""Cost of paired-end random PBAT (walt_map_pe_rpbat_batch) on the hg19-like genome: one process, one 4-strand index,
one resident batch of 2 x L pairs (tools/synth.py's make_pairs, the mates of a fixed half exchanged: pairs of either
orientation), timed three ways on the same batch and stream:
  * the plain paired-end call          (walt_map_pe_batch_device(m1, m2))
  * the mate-exchanged call            (walt_map_pe_batch_device(m2, m1): what -P maps)
  * the random-PBAT call               (walt_map_pe_rpbat_batch_device)
and a uniform sample of the batch checked against the rule of include/walt_amd.h applied to the oracle's two
orientations (tests/test_pe_rpbat_cpu.py).  The merge kernel's own time comes from running this tool under
    rocprofv3 --kernel-trace --stats -d <dir> -- python3 tools/pe_rpbat_bench.py ...
(k_pe_rpbat_merge in the kernel statistics).  Prints one JSON line.

  python3 tools/pe_rpbat_bench.py [--pairs 50000000] [--read-len 100] [--steps 3] [--warmup 1] [--sample 20000]"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)


def log(msg):
    print("[pe_rpbat_bench] " + msg, file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=50_000_000)
    ap.add_argument("--read-len", type=int, default=100)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--genome-mbp", type=float, default=None, help="synthetic genome size (default: full scale)")
    ap.add_argument("--sample", type=int, default=20_000, help="pairs of the batch the oracle checks")
    ap.add_argument("--max-mismatches", type=int, default=6)
    ap.add_argument("--bucket", type=int, default=5000)
    ap.add_argument("--top-k", type=int, default=50)
    ap.add_argument("--frag-range", type=int, default=1000)
    args = ap.parse_args()

    import torch
    import synth
    import walt_amd
    import bench
    import test_pe_rpbat_cpu as rule_of
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    scale = 1.0 if args.genome_mbp is None else args.genome_mbp * 1e6 / synth.HG19_TOTAL
    t0 = time.perf_counter()
    genome_ascii, lens, names = synth.make_genome(torch, dev, scale, seed=2, kind="hg19like")
    torch.cuda.synchronize()
    log("genome: %d bp in %d sequences (%.1f s)" % (sum(lens), len(lens), time.perf_counter() - t0))
    torch.cuda.empty_cache()
    t0 = time.perf_counter()
    idx = walt_amd.Index.build_device(genome_ascii.data_ptr(), lens, names, device=0, strands=walt_amd.STRANDS_ALL)
    log("index (4 strands): %.1f GB in HBM (%.1f s)" % (idx.device_bytes / 1e9, time.perf_counter() - t0))
    n, L = args.pairs, args.read_len
    a1, a2, d_off = synth.make_pairs(torch, dev, genome_ascii, n, L, seed=2000 + L)
    del genome_ascii
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    swap = torch.rand(n, generator=gen, device=dev) < 0.5  # the pairs whose A-rich mate comes first
    a1, a2 = a1.view(n, L), a2.view(n, L)
    d1 = torch.where(swap[:, None], a2, a1).reshape(-1).contiguous()
    d2 = torch.where(swap[:, None], a1, a2).reshape(-1).contiguous()
    del a1, a2
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    mm, b, k, fr = args.max_mismatches, args.bucket, args.top_k, args.frag_range
    d_out = torch.zeros(n * 64, dtype=torch.uint8, device=dev)
    d_conv = torch.zeros(2 * n, dtype=torch.uint8, device=dev)
    d_stats = torch.zeros(8, dtype=torch.int64, device=dev)
    ws = idx.pe_rpbat_workspace_bytes(n, L, k)  # also what the plain calls get: they take the same pass geometry
    d_ws = torch.empty(ws, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def plain(x, y):
        idx.map_pe_batch_device(x.data_ptr(), d_off.data_ptr(), y.data_ptr(), d_off.data_ptr(), n, L, d_out.data_ptr(),
                                d_stats.data_ptr(), d_ws.data_ptr(), ws, stream=stream, max_mismatches=mm, b=b, top_k=k,
                                frag_range=fr)

    def rpbat():
        idx.map_pe_rpbat_batch_device(d1.data_ptr(), d_off.data_ptr(), d2.data_ptr(), d_off.data_ptr(), n, L,
                                      d_out.data_ptr(), d_conv.data_ptr(), d_stats.data_ptr(), d_ws.data_ptr(), ws,
                                      stream=stream, max_mismatches=mm, b=b, top_k=k, frag_range=fr)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        walt_amd.Index.check_batch(d_ws.data_ptr(), stream)
        return float(np.median(ms)), ms

    t_ms, t_all = timed(lambda: plain(d1, d2))
    log("plain call: %.1f ms (median of %s)" % (t_ms, ["%.1f" % x for x in t_all]))
    a_ms, a_all = timed(lambda: plain(d2, d1))
    log("mate-exchanged call: %.1f ms (median of %s)" % (a_ms, ["%.1f" % x for x in a_all]))
    d_stats.zero_()
    rp_ms, rp_all = timed(rpbat)
    log("random-PBAT call: %.1f ms (median of %s); sum of the two: %.1f ms" % (rp_ms, ["%.1f" % x for x in rp_all],
                                                                             t_ms + a_ms))
    st = d_stats.cpu().numpy() // (args.warmup + args.steps)
    rec = d_out.view(torch.int32).view(n, 16)
    bt = rec[:, 8]
    conv = d_conv.view(n, 2)
    a_first = conv[:, 0] == ord("A")
    uniq = bt == 1
    share = {
        "unique": float(uniq.float().mean()), "ambiguous": float((bt >= 2).float().mean()),
        "unmapped": float((bt == 0).float().mean()), "mate1_conv_A": float(a_first.float().mean()),
        "unique_pairs_orientation_as_made": float((a_first[uniq] == swap[uniq]).float().mean()),
    }
    log("shares: %s" % share)

    # exactness: a uniform sample against the rule on the oracle's two orientations
    m = min(args.sample, n)
    sel = (torch.arange(m, device=dev, dtype=torch.int64) * n) // m
    h1 = d1.view(n, L)[sel].cpu().numpy().copy()
    h2 = d2.view(n, L)[sel].cpu().numpy().copy()
    got = d_out.view(n, 64)[sel].cpu().numpy().reshape(-1).view(walt_amd.pair_result_dtype)
    got_conv = conv[sel].cpu().numpy()
    del d1, d2, d_out, d_ws
    torch.cuda.empty_cache()
    t0 = time.perf_counter()
    jobs = [dict(m1=x, m2=y, m=m, nu=m, read_len=L, max_mm=mm, b=b, top_k=k, frag_range=fr) for x, y in ((h1, h2), (h2, h1))]
    bench.oracle_pe_jobs(SimpleNamespace(walt_amd=walt_amd), idx, jobs, lens)
    start = np.zeros(len(lens) + 1, dtype=np.uint32)
    start[1:] = np.cumsum(lens, dtype=np.uint64).astype(np.uint32)
    db = SimpleNamespace(start_index=start, n_chrom=len(lens))
    ln = np.full(m, L, dtype=np.int64)
    mins = [rule_of.pair_min_mm(db, (j["ranked"][0], j["counts"][0], j["ranked"][1], j["counts"][1]), ln, ln, mm, fr)
            for j in jobs]
    mins = [np.where(j["out"]["best_times"] >= 1, mn, -1) for j, mn in zip(jobs, mins)]  # defined where best_times >= 1
    want, want_conv, rule = rule_of.pe_rpbat_rule(jobs[0]["out"], jobs[1]["out"], mins[0], mins[1])
    try:
        rule_of.compare(got, got_conv, want, want_conv, "sample")
        same, diff = True, ""
    except AssertionError as e:
        same, diff = False, str(e)[:300]
    log("oracle over %d sampled pairs: %s (%.1f s); rules 1-5: %s" % (
        m, "identical" if same else "DIFFERENT: " + diff, time.perf_counter() - t0, list(np.bincount(rule, minlength=6)[1:])))
    idx.close()
    print(json.dumps({
        "tool": "pe_rpbat_bench", "pairs": n, "read_len": L, "max_mismatches": mm, "b": b, "top_k": k,
        "frag_range": fr, "genome_bp": int(sum(lens)), "steps": args.steps, "warmup": args.warmup,
        "plain_ms": t_ms, "exchanged_ms": a_ms, "rpbat_ms": rp_ms, "sum_plain_exchanged_ms": t_ms + a_ms,
        "rpbat_over_sum": rp_ms / (t_ms + a_ms), "plain_ms_all": t_all, "exchanged_ms_all": a_all,
        "rpbat_ms_all": rp_all,
        "rpbat_stats_per_call": {"mate1": {"too_short": int(st[0]), "probes": int(st[1]), "candidates": int(st[2]),
                                           "big_regions": int(st[3])},
                                 "mate2": {"too_short": int(st[4]), "probes": int(st[5]), "candidates": int(st[6]),
                                           "big_regions": int(st[7])}},
        "shares": share, "oracle_sample": m, "oracle_identical": bool(same),
        "oracle_rules_1_to_5": [int(x) for x in np.bincount(rule, minlength=6)[1:]],
    }))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
