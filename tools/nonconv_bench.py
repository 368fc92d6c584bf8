#!/usr/bin/env python3
"""Cost of keeping non-converted reads out of the counts (walt_nonconv_batch_device, walt_meth_nonconv_batch_device)
beside the counting call, on the hg19-like genome: one process, one resident batch of single-end reads (tools/synth.py's
make_reads) mapped once, then timed on the same batch and stream, alternating, by device events after a warm-up:
  * the plain counting call                (walt_meth_pileup_batch_trim_device with a pile-up, batch totals, no calls out)
  * the judging kernel alone on the calls  (walt_nonconv_batch_device)
  * calling and judging in one step        (walt_meth_nonconv_batch_device)
  * the whole filtered sequence            (the one-step form, then the counting call with the verdicts as skip bytes)
The judging kernel's rate is over the bytes it reads and writes -- calls, offsets, records, tally, verdict -- and is put
beside the streaming rate given with --stream-rate (bytes/s, as tools/stream_calib.hip measures it on the device in the same
session).  Every verdict and tally is checked against the rule of tests/test_gpu_nonconv.py, evaluated on the device over
all reads, and a sample of reads against that file's plain loops themselves.

--plain-only times the counting call alone and needs no entry point of this feature: run on a built tree of the parent
commit (--package-root <that tree>) it gives the parent's number on the same batch; --parent-json puts that file's
figures into this run's line.  Prints one JSON line; --out also writes it to a file (profiles/nonconv_hg19like.json).

  python3 tools/nonconv_bench.py [--reads 50000000] [--read-len 100] [--steps 20] [--warmup 2] [--stream-rate 4.0e12]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)


def log(msg):
    print("[nonconv_bench] " + msg, file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=50_000_000)
    ap.add_argument("--read-len", type=int, default=100)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--genome-mbp", type=float, default=None, help="synthetic genome size (default: full scale)")
    ap.add_argument("--max-mismatches", type=int, default=6)
    ap.add_argument("--bucket", type=int, default=5000)
    ap.add_argument("--rule", default="3,0,0,0", help="min_meth,min_run,min_percent,min_total")
    ap.add_argument("--stream-rate", type=float, default=None, help="the device's streaming rate in bytes/s (tools/stream_calib.hip)")
    ap.add_argument("--plain-only", action="store_true", help="time the counting call alone (any library that has it)")
    ap.add_argument("--parent-json", default=None, help="the --plain-only line of the parent commit's library on the same batch")
    ap.add_argument("--package-root", default=ROOT, help="the tree whose walt_amd package and library are used (default: this one)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_root))

    import torch
    import synth
    import walt_amd
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
    n, L = args.reads, args.read_len
    d_bases, _ = synth.make_reads(torch, dev, genome_ascii, n, L, seed=1000, ag=False)
    del genome_ascii
    d_off = torch.arange(n + 1, device=dev, dtype=torch.int64) * L
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    d_out = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    d_stats = torch.zeros(4, dtype=torch.int64, device=dev)
    ws = walt_amd.lib().walt_se_workspace_bytes(n, L)
    d_ws = torch.empty(ws, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    idx.map_se_batch_device(d_bases.data_ptr(), d_off.data_ptr(), n, L, d_out.data_ptr(), d_stats.data_ptr(), d_ws.data_ptr(), ws,
                            stream=stream, ag_wildcard=False, max_mismatches=args.max_mismatches, b=args.bucket)
    torch.cuda.synchronize()
    walt_amd.Index.check_batch(d_ws.data_ptr(), stream)
    del d_ws
    torch.cuda.empty_cache()
    pile = idx.pileup()
    d_mstats = torch.zeros(9, dtype=torch.int64, device=dev)
    d_filt = torch.zeros(n, dtype=torch.uint8, device=dev)
    L_ = walt_amd.lib()

    def counting(d_skip=None):
        # the C call itself, so that a library without this feature's entry points runs it too
        rc = L_.walt_meth_pileup_batch_trim_device(idx.handle, pile.handle, d_bases.data_ptr(), d_off.data_ptr(), n, d_out.data_ptr(), 16,
                                                   None, 1, ord("T"), None, None, None, d_mstats.data_ptr(), d_skip, 1, None, None, 0, 0, 0,
                                                   stream)
        assert rc == 0, L_.walt_last_error()

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    med = lambda v: float(np.median(v))
    out = {"tool": "nonconv_bench", "library": "this tree" if os.path.abspath(args.package_root) == ROOT else "the tree given with --package-root", "reads": n, "read_len": L, "genome_bp": int(sum(lens)),
           "steps": args.steps, "warmup": args.warmup}
    if args.plain_only:
        for _ in range(args.warmup):
            counting()
        torch.cuda.synchronize()
        t = [once(counting) for _ in range(args.steps)]
        out.update({"plain_only": True, "counting_ms": med(t), "counting_ms_min": min(t), "counting_ms_max": max(t), "counting_ms_all": t})
    else:
        import test_gpu_nonconv as rule_of
        rule = tuple(int(v) for v in args.rule.split(","))
        r = walt_amd.nonconv_rule(*rule)
        d_calls = torch.zeros(n * L, dtype=torch.uint8, device=dev)
        d_tally = torch.zeros((n, 4), dtype=torch.int16, device=dev)

        def judge():
            idx.nonconv_batch_device(d_calls.data_ptr(), d_off.data_ptr(), n, d_out.data_ptr(), r, d_filt.data_ptr(), d_tally=d_tally.data_ptr(),
                                     stream=stream)

        def one_step():
            idx.meth_nonconv_batch_device(d_bases.data_ptr(), d_off.data_ptr(), n, d_out.data_ptr(), r, d_calls.data_ptr(), d_filt.data_ptr(),
                                          d_tally=d_tally.data_ptr(), stream=stream)

        def sequence():
            one_step()
            counting(d_filt.data_ptr())

        legs = {"counting": counting, "judge": judge, "one_step": one_step, "sequence": sequence}
        one_step()
        for _ in range(args.warmup):
            for fn in legs.values():
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in legs}
        for _ in range(args.steps):  # alternating, so that clock and temperature drift hit all legs alike
            for k, fn in legs.items():
                t[k].append(once(fn))
        # the rule over all reads, on the device: one pass over the read positions for the run
        times = d_out.view(torch.int32).view(n, 4)[:, 1]
        rows = d_calls.view(n, L)
        judged = times == 1
        meth = torch.zeros(n, dtype=torch.int32, device=dev)
        total = torch.zeros(n, dtype=torch.int32, device=dev)
        run = torch.zeros(n, dtype=torch.int32, device=dev)
        cur = torch.zeros(n, dtype=torch.int32, device=dev)
        for i in range(L):
            col = rows[:, i]
            up = (col == ord("H")) | (col == ord("X"))
            low = (col == ord("h")) | (col == ord("x"))
            meth += up
            total += up | low
            cur = torch.where(up, cur + 1, torch.where(low, torch.zeros_like(cur), cur))
            run = torch.maximum(run, cur)
        floor_total = max(rule[3], 1)
        verdict = torch.zeros(n, dtype=torch.bool, device=dev)
        if rule[0]:
            verdict |= meth >= rule[0]
        if rule[1]:
            verdict |= run >= rule[1]
        if rule[2]:
            verdict |= (total >= floor_total) & (100 * meth.long() >= rule[2] * total.long())
        verdict &= judged
        z = torch.zeros_like(meth)
        got_t = d_tally.view(n, 4).to(torch.int32)
        identical = bool(torch.equal(d_filt.bool(), verdict) and torch.equal(got_t[:, 0], torch.where(judged, meth, z)) and
                         torch.equal(got_t[:, 1], torch.where(judged, total, z)) and torch.equal(got_t[:, 2], torch.where(judged, run, z)) and
                         not bool(got_t[:, 3].any()))
        m = min(n, 2000)  # and a sample through the plain loops themselves
        want_f, want_t = rule_of.expected_verdicts(d_calls[:m * L].cpu().numpy(), np.arange(m + 1) * L, times[:m].cpu().numpy(), rule)
        sample_ok = bool(np.array_equal(d_filt[:m].cpu().numpy(), want_f) and np.array_equal(got_t[:m, :3].cpu().numpy().astype(np.int64), want_t))
        log("verdicts and tallies of %d reads: %s; sample of %d through the plain loops: %s" % (
            n, "identical to the rule" if identical else "DIFFER", m, "identical" if sample_ok else "DIFFERS"))
        judge_bytes = n * L + 8 * (n + 1) + 16 * n + 9 * n
        judge_rate = judge_bytes / (med(t["judge"]) * 1e-3)
        parent = None
        if args.parent_json:
            with open(args.parent_json) as f:
                parent = json.loads(f.read())
        out.update({"rule": list(rule), "counting_ms": med(t["counting"]), "counting_ms_min": min(t["counting"]), "counting_ms_max": max(t["counting"]),
                    "judge_ms": med(t["judge"]), "one_step_ms": med(t["one_step"]), "sequence_ms": med(t["sequence"]),
                    "sequence_minus_counting_ms": med(t["sequence"]) - med(t["counting"]),
                    "sequence_over_counting": med(t["sequence"]) / med(t["counting"]),
                    "judge_bytes": judge_bytes, "judge_bytes_per_s": judge_rate, "stream_bytes_per_s": args.stream_rate,
                    "judge_share_of_stream": None if not args.stream_rate else judge_rate / args.stream_rate,
                    "judged_reads": int(judged.sum()), "filtered_reads": int(verdict.sum()), "verdicts_identical": identical,
                    "sample_identical": sample_ok,
                    "parent_counting_ms": None if parent is None else parent["counting_ms"],
                    "parent_counting_ms_min": None if parent is None else parent["counting_ms_min"],
                    "parent_counting_ms_max": None if parent is None else parent["counting_ms_max"],
                    "parent_library": None if parent is None else parent["library"],
                    "sequence_over_parent_counting": None if parent is None else med(t["sequence"]) / parent["counting_ms"],
                    "counting_ms_all": t["counting"], "judge_ms_all": t["judge"], "one_step_ms_all": t["one_step"],
                    "sequence_ms_all": t["sequence"]})
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    pile.close()
    idx.close()
    return 0 if args.plain_only or (out["verdicts_identical"] and out["sample_identical"]) else 1


if __name__ == "__main__":
    sys.exit(main())
