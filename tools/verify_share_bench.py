#!/usr/bin/env python3
"""How often the single-end dense verifier is given the same region, and what grouping the items by region does to
a step (option se_verify_share, walt_amd/csrc/map_se.hip): one process, the genome and reads of bench.py's headline leg
(tools/synth.py: hg19-like genome, seed 2; 100-base reads, seed 1000), one resident batch, device events.

For every (chunk, round) of the staged heavy pass the library keeps two 64-bit counters at the end of the workspace:
the records of all items (sum of size) and the records of all units (sum of size per unit); their ratio is the record
traffic grouping removes.  The tool runs
  * se_verify_share = 2 (items grouped and counted, verified one by one) with units of at most 2, 4, 8 and 64 items
    (64 = one slice of a bucket: as good as unbounded) -- the counters per round;
  * se_verify_share = 0, 1 (units of at most 4) and 2 -- ms per step and per kernel group (walt_profile_detail), in
    turn, --rounds times; every variant's records and statistics are compared with those of se_verify_share = 0.
Prints one JSON line; --out also writes it to a file (profiles/verify_share_hg19like.json).

  python3 tools/verify_share_bench.py [--reads 50000000] [--read-len 100] [--steps 3] [--warmup 1] [--rounds 2] [--opt se_pipe=0]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def log(msg):
    print("[verify_share_bench] " + msg, file=sys.stderr, flush=True)


def share_counters(torch, d_ws, kpat):
    """[chunk][round] -> (records of all items, records of all units): the last 8 * kpat * 16 bytes of the workspace"""
    end = d_ws.numel() // 16 * 16
    raw = d_ws[end - 8 * kpat * 16:end].view(torch.int64).cpu().numpy().reshape(8, kpat, 2)
    return raw


def rode_along(torch, d_ws, n, read_len, kpat):
    """control word 7 of every (chunk, round): items that rode along in a unit (bench.py's offset of the control words)"""
    stride = (n + 63) // 64 * 64
    h_off = (64 * 4 + 256 * 16 * 8 + 3 * stride * 4 + ((n * read_len) // 16 + 10) * 4 + 15) // 16 * 16
    hctl = d_ws[h_off:h_off + 4 * 64 * kpat].view(torch.int32).cpu().numpy().reshape(8, kpat, 8)
    return hctl[:, :, 7].astype(np.int64), hctl[:, :, 0].astype(np.int64) + hctl[:, :, 5].astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=50_000_000)
    ap.add_argument("--read-len", type=int, default=100)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=2, help="times the timed variants are taken in turn")
    ap.add_argument("--genome-mbp", type=float, default=None, help="synthetic genome size (default: full scale)")
    ap.add_argument("--max-mismatches", type=int, default=6)
    ap.add_argument("--bucket", type=int, default=5000)
    ap.add_argument("--opt", action="append", default=[], help="name=value: an index option for every run (se_pipe=0: one stream)")
    ap.add_argument("--counters-only", action="store_true", help="skip the timed variants")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()

    import torch
    import synth
    import walt_amd
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    kpat = 3
    scale = 1.0 if args.genome_mbp is None else args.genome_mbp * 1e6 / synth.HG19_TOTAL
    t0 = time.perf_counter()
    genome_ascii, lens, names = synth.make_genome(torch, dev, scale, seed=2, kind="hg19like")
    torch.cuda.synchronize()
    log("genome: %d bp in %d sequences (%.1f s)" % (int(sum(lens)), len(lens), time.perf_counter() - t0))
    torch.cuda.empty_cache()
    idx = walt_amd.Index.build_device(genome_ascii.data_ptr(), lens, names, device=0, strands=walt_amd.STRANDS_CT)
    n, L = args.reads, args.read_len
    d_bases, _ = synth.make_reads(torch, dev, genome_ascii, n, L, seed=1000, ag=False)
    del genome_ascii
    d_off = torch.arange(n + 1, device=dev, dtype=torch.int64) * L
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    log("index and %d reads ready (%.1f s)" % (n, time.perf_counter() - t0))
    for o in args.opt:
        name, value = o.split("=")
        idx.set_option(name, int(value))
    d_out = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    d_stats = torch.zeros(4, dtype=torch.int64, device=dev)
    ws = walt_amd.lib().walt_se_workspace_bytes(n, L)
    d_ws = torch.empty(ws, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    idx.profile_enable(True)

    def step():
        d_stats.zero_()
        idx.map_se_batch_device(d_bases.data_ptr(), d_off.data_ptr(), n, L, d_out.data_ptr(), d_stats.data_ptr(), d_ws.data_ptr(), ws,
                                stream=stream, ag_wildcard=False, max_mismatches=args.max_mismatches, b=args.bucket)

    def variant(share, r):
        idx.set_option("se_verify_share", share)
        idx.set_option("se_share_r", r)

    out = {"tool": "verify_share_bench", "reads": n, "read_len": L, "genome_bp": int(sum(lens)), "options": args.opt,
           "steps": args.steps, "warmup": args.warmup, "workspace_bytes": int(ws)}
    # ---- the base line's records
    variant(0, 0)
    step()
    torch.cuda.synchronize()
    idx.check_batch(d_ws.data_ptr(), stream)
    base_out, base_stats = d_out.clone(), d_stats.clone()
    # ---- the counters
    counters = {}
    for r in (2, 4, 8, 64):
        variant(2, r)
        step()
        torch.cuda.synchronize()
        idx.check_batch(d_ws.data_ptr(), stream)
        c = share_counters(torch, d_ws, kpat)
        rode, items = rode_along(torch, d_ws, n, L, kpat)
        used = [ch for ch in range(8) if c[ch].any()]
        per_round = [{"round": rd, "records_of_items": int(c[used, rd, 0].sum()), "records_of_units": int(c[used, rd, 1].sum()),
                      "items": int(items[used, rd].sum()), "rode_along": int(rode[used, rd].sum())} for rd in range(kpat)]
        ri, ru = int(c[:, :, 0].sum()), int(c[:, :, 1].sum())
        counters["r%d" % r] = {"records_of_items": ri, "records_of_units": ru, "units_over_items": ru / ri if ri else None,
                               "items": int(items.sum()), "rode_along": int(rode.sum()), "chunks": len(used), "rounds": per_round,
                               "records_identical": bool(torch.equal(d_out, base_out)), "stats_identical": bool(torch.equal(d_stats, base_stats))}
        log("units of at most %d: records of items %d, of units %d (%.3f); %d of %d items rode along" % (
            r, ri, ru, ru / ri if ri else 0.0, int(rode.sum()), int(items.sum())))
    out["counters"] = counters
    # ---- the timed variants, in turn
    if not args.counters_only:
        variants = [("share0", 0, 0), ("share1", 1, 0), ("share2_r4", 2, 4)]
        timed = {k: {"map_ms": [], "detail_ms": []} for k, _, _ in variants}
        for rnd in range(args.rounds):
            for key, share, r in variants:
                variant(share, r)
                for _ in range(args.warmup):
                    step()
                for _ in range(args.steps):
                    step()
                    _, m_ms = idx.profile_last()
                    timed[key]["map_ms"].append(m_ms)
                    timed[key]["detail_ms"].append(idx.profile_detail())
                torch.cuda.synchronize()
                idx.check_batch(d_ws.data_ptr(), stream)
                timed[key]["records_identical"] = bool(torch.equal(d_out, base_out)) and timed[key].get("records_identical", True)
                timed[key]["stats_identical"] = bool(torch.equal(d_stats, base_stats)) and timed[key].get("stats_identical", True)
        for key in timed:
            v = timed[key]
            v["map_ms_median"] = float(np.median(v["map_ms"]))
            v["map_ms_min"], v["map_ms_max"] = float(min(v["map_ms"])), float(max(v["map_ms"]))
            v["detail_ms_median"] = dict(zip(("pass1", "heavy_stages", "se_verify", "literal"), np.median(np.array(v["detail_ms"]), axis=0).tolist()))
            log("%s: map %.2f ms (%.2f .. %.2f), groups %s, records %s" % (key, v["map_ms_median"], v["map_ms_min"], v["map_ms_max"],
                                                                          {k: round(x, 2) for k, x in v["detail_ms_median"].items()},
                                                                          "identical" if v["records_identical"] and v["stats_identical"] else "DIFFER"))
        out["timed"] = timed
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    idx.close()
    ok = all(v["records_identical"] and v["stats_identical"] for v in counters.values())
    if not args.counters_only:
        ok = ok and all(v["records_identical"] and v["stats_identical"] for v in out["timed"].values())
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
