#!/usr/bin/env python3
"""Randomised parity soak on the GPU box: fresh random genomes (many short chromosomes, planted repeats,
low-entropy stretches) and read sets with random options, mapped through the C ABI and compared record by
record with the oracle (tests/refio.py; test infrastructure).  Runs until --seconds are used up.

  python3 tools/soak.py --seconds 300 [--seed0 1] [--pattern 3|5|7]
Prints one summary line; exits non-zero at the first difference (with the offending case)."""
import argparse
import os
import random
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def make_genome(rng, pattern, many=False):
    """many: also draw sequence counts beyond what the kernels' table of chromosome starts holds whole (1,023) and
    beyond its five-word path (4,092; walt_amd/csrc/chrom_core.h), with short sequences so that a genome costs the same"""
    n_chrom = rng.choice([3, 12, 60, 250, 900, 1100, 2600, 4500, 9000] if many else [3, 12, 60, 250, 900])
    low = rng.random() < 0.4
    alphabet = rng.choice(["TTTTTCCAG", "TTCCCAAGG"]) if low else "ACGT"
    unit = "".join(rng.choice(alphabet) for _ in range(300))
    seqs = []
    for i in range(n_chrom):
        L = rng.choice([36, 37, 38, 40, 52, 90, 150] if n_chrom > 1000 else [36, 37, 38, 40, 52, 90, 150, 300, 700, 2000, 6000])
        s = [rng.choice(alphabet) for _ in range(L)]
        if L >= 150 and rng.random() < 0.6:
            p = rng.randrange(0, L - 60)
            ln = min(len(unit), L - p)
            s[p:p + ln] = unit[:ln]
        seqs.append(("c%d" % i, "".join(s)))
    seqs.append(("big", "".join(rng.choice(alphabet) for _ in range(20000)) + unit * 3))
    if rng.random() < 0.12:  # now and then a few Mbp, so that buckets and directory slots fill up
        big = np.random.default_rng(rng.randrange(1 << 30)).integers(0, len(alphabet), rng.choice([1500000, 4000000]))
        seqs.append(("huge", "".join(np.array(list(alphabet))[big])))
    return seqs


def sample(rng, seqs, n, conv, lengths, refio):
    a, b = ("C", "T") if conv == "CT" else ("G", "A")
    out = []
    while len(out) < n:
        _, g = seqs[rng.randrange(len(seqs))]
        L = rng.choice(lengths)
        if len(g) < L:
            continue
        p = rng.randrange(0, len(g) - L + 1)
        if rng.random() < 0.3:
            p = rng.choice([0, len(g) - L, max(0, len(g) - L - 1)])
        s = g[p:p + L]
        if rng.random() < 0.5:
            s = refio.revcomp(s)
        s = "".join(b if (c == a and rng.random() < 0.9) else c for c in s)
        rate = rng.choice([0.0, 0.01, 0.04])
        out.append("".join(rng.choice("ACGT") if rng.random() < rate else c for c in s))
    return out


class SoakMismatch(AssertionError):
    pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=300)
    ap.add_argument("--seed0", type=int, default=1)
    ap.add_argument("--pattern", type=int, default=3, choices=[3, 5, 7])
    ap.add_argument("--genomes", type=int, default=0, help="stop after this many genomes (0: when --seconds are used up)")
    args = ap.parse_args()
    try:
        print(run_soak(args.seconds, args.seed0, args.pattern, args.genomes or None))
    except SoakMismatch as e:
        print(e)
        sys.exit(1)


def rode_along(walt_amd, idx, reads, ag, m, b, pattern):
    """Items of the grouped dense verifier that rode along in a unit (map_se.hip k_se_share_cut: control word 7 of every
    (chunk, round) of the staged pass, summed): one more call of the batch through the device form, whose workspace the
    caller owns and can read.  The records are not compared again."""
    import torch
    dev = torch.device("cuda:0")
    bases, offsets = walt_amd.pack_reads(reads)
    n = offsets.size - 1
    max_len = int((offsets[1:] - offsets[:-1]).max())
    d_bases = torch.from_numpy(bases).to(dev)
    d_off = torch.from_numpy(offsets.astype(np.int64)).to(dev)
    d_out = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    d_stats = torch.zeros(4, dtype=torch.int64, device=dev)
    ws = walt_amd.lib(pattern).walt_se_workspace_bytes(n, max_len)
    d_ws = torch.empty(ws, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    idx.map_se_batch_device(d_bases.data_ptr(), d_off.data_ptr(), n, max_len, d_out.data_ptr(), d_stats.data_ptr(), d_ws.data_ptr(), ws,
                            stream=stream, ag_wildcard=ag, max_mismatches=m, b=b)
    torch.cuda.synchronize()
    walt_amd.Index.check_batch(d_ws.data_ptr(), stream)
    stride = (n + 63) // 64 * 64  # (bench.py's offset of the staged pass's control words; 8 words per (chunk, round), 8 x pattern of them)
    h_off = (64 * 4 + 256 * 16 * 8 + 3 * stride * 4 + ((n * max_len) // 16 + 10) * 4 + 15) // 16 * 16
    hctl = d_ws[h_off:h_off + 4 * 64 * pattern].view(torch.int32).cpu().numpy().reshape(8 * pattern, 8)
    return int(hctl[:, 7].sum())


def run_soak(seconds, seed0=1, pattern=3, max_genomes=None):
    """Genomes seed0, seed0 + 1, ... until `seconds` are used up or `max_genomes` are done; returns the summary line,
    raises SoakMismatch at the first difference (tests/test_gpu_soak.py runs a fixed set of seeds this way)."""
    from types import SimpleNamespace
    args = SimpleNamespace(seconds=seconds, seed0=seed0, pattern=pattern)
    import refio
    import walt_amd
    refio.set_pattern(args.pattern)
    walt_amd.set_pattern(args.pattern)
    lo, hi = refio.MIN_READ_LEN[args.pattern], min(refio.MAX_READ_LEN[args.pattern], 260)
    t_end = time.time() + args.seconds
    base = "/dev/shm" if os.path.isdir("/dev/shm") else None
    cases = reads_total = pairs_total = 0
    seed = args.seed0
    t_note = time.time()
    while time.time() < t_end and (max_genomes is None or cases < max_genomes):
        if time.time() - t_note > 60:  # a sign of life (runs under a watchdog that takes minutes of silence for a hang)
            print("soak: %d genomes so far, no difference" % cases, file=sys.stderr, flush=True)
            t_note = time.time()
        rng = random.Random(seed)
        tmp = tempfile.mkdtemp(prefix="walt_soak_", dir=base)
        try:
            seqs = make_genome(rng, args.pattern)
            fa = os.path.join(tmp, "g.fa")
            with open(fa, "w") as f:
                for nm, s in seqs:
                    f.write(">%s\n%s\n" % (nm, s))
            path = os.path.join(tmp, "g.dbindex")
            walt_amd.makedb(fa, path, threads=4)
            db = refio.DbIndex(path)
            D = rng.choice([-1, 24, 26, 29])
            if rng.random() < 0.3:
                os.environ["WALT_AMD_TABLE"] = "1"
            else:
                os.environ.pop("WALT_AMD_TABLE", None)
            idx = walt_amd.Index.open(path, device=0, dir_bits=D)
            # a third of the genomes on one or two blocks: every wavefront of the staged kernels then walks through several
            # windows of its list (the read hand-out of k_se_stage), which 1,500 reads on the full grid never do
            g_opt = rng.choice([0, 0, 0, 0, 1, 2])
            if g_opt:
                idx.set_option("grid", g_opt)
            # a quarter of the genomes with the paired-end literal round seed by seed (default: one launch when the list
            # is short, map_pe.hip k_pe_stage); drawn from a generator of its own so that a seed's genome and reads stay
            if random.Random(seed * 7919 + 13).random() < 0.25:
                idx.set_option("pe_lit_fuse", 0)
            # the dense items grouped by region (default) or verified one by one (map_se.hip k_se_verify_shared); a
            # generator of its own again
            share = random.Random(seed * 104729 + 7).choice([1, 1, 0])
            idx.set_option("se_verify_share", share)
            rode = 0
            lengths = [lo + 2, lo + 3, 40, 45, 60, 100, 100, 100, 131, 140, min(150, hi), min(200, hi), hi]
            # the kernels are instantiated per read-length class (up to 112, 128, 160 ... bases: the batch's longest read
            # selects the instance): some genomes get batches that stop at 112 or 128 bases
            cls = rng.choice(["all", "all", "le112", "le128"])
            if cls == "le112":
                lengths = [x for x in lengths if x <= 112] + [90, 96, 104, 110, 112]
            elif cls == "le128":
                lengths = [x for x in lengths if x <= 128] + [100, 113, 119, 120, 125, 128]
            m, b, k = rng.choice([0, 2, 6, 10]), rng.choice([2, 30, 5000]), rng.choice([2, 5, 50, 300])
            for conv, ag in (("CT", False), ("GA", True)):
                reads = sample(rng, seqs, 1500, conv, lengths, refio)
                want, _ = refio.oracle_se(db, reads, ag=ag, max_mm=m, b=b)
                got, _ = idx.map_se_batch(*walt_amd.pack_reads(reads), ag_wildcard=ag, max_mismatches=m, b=b)
                for f in ("genome_pos", "times", "strand", "mismatch"):
                    if not np.array_equal(got[f], want[f]):
                        bad = int(np.nonzero(got[f] != want[f])[0][0])
                        raise SoakMismatch("MISMATCH seed %d %s field %s read %d (%s) D=%d m=%d b=%d" % (seed, conv, f, bad, reads[bad], D, m, b))
                reads_total += len(reads)
                if share == 1:
                    rode += rode_along(walt_amd, idx, reads, ag, m, b, args.pattern)
            if share == 1:  # whether grouping happened at all on this genome (none on the routes of reads above 128 bases)
                print("soak: seed %d, se_verify_share = 1: %d items rode along in a unit (%s)" % (seed, rode, cls), file=sys.stderr, flush=True)
            s1 = sample(rng, seqs, 500, "CT", lengths, refio)
            s2 = sample(rng, seqs, 500, "GA", lengths, refio)
            L = rng.choice([200, 1000])
            res, _ = idx.map_pe_batch(*walt_amd.pack_reads(s1), *walt_amd.pack_reads(s2), max_mismatches=m, b=b, top_k=k,
                                      frag_range=L)
            wantp, _, _ = refio.oracle_pe(db, s1, s2, max_mm=m, b=b, top_k=k, frag_range=L)
            for f in ("best_times", "frag_len", "pair_mm", "best_i", "best_j"):
                if not np.array_equal(res[f], wantp[f]):
                    bad = int(np.nonzero(res[f] != wantp[f])[0][0])
                    raise SoakMismatch("MISMATCH seed %d paired-end field %s pair %d D=%d m=%d b=%d k=%d L=%d" % (seed, f, bad, D, m, b, k, L))
            for mate in ("m1", "m2"):
                for f in ("genome_pos", "times", "strand", "mismatch"):
                    if not np.array_equal(res[mate][f], wantp[mate][f]):
                        raise SoakMismatch("MISMATCH seed %d paired-end %s.%s D=%d m=%d b=%d k=%d L=%d" % (seed, mate, f, D, m, b, k, L))
            pairs_total += len(s1)
            idx.close()
            cases += 1
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
        seed += 1
    os.environ.pop("WALT_AMD_TABLE", None)
    return "soak ok: pattern %d, %d genomes, %d single-end reads and %d pairs identical to the oracle (seeds %d..%d)" % (
        args.pattern, cases, reads_total, pairs_total, args.seed0, seed - 1)


def run_soak_rpbat(seeds, pattern=3):
    """Random PBAT (walt_map_se_rpbat_batch) on the genomes of `seeds`: each read drawn T-rich or A-rich at random, the
    GPU's records and conversions compared with the rule of include/walt_amd.h applied to the oracle's C->T and G->A
    runs.  Returns the summary line, raises SoakMismatch at the first difference (tests/test_gpu_rpbat_soak.py)."""
    import refio
    import walt_amd
    refio.set_pattern(pattern)
    walt_amd.set_pattern(pattern)
    lo, hi = refio.MIN_READ_LEN[pattern], min(refio.MAX_READ_LEN[pattern], 260)
    base = "/dev/shm" if os.path.isdir("/dev/shm") else None
    reads_total = 0
    try:
        for seed in seeds:
            rng = random.Random(seed * 104729 + 1)  # a generator of its own: run_soak's draws for a seed stay as they are
            tmp = tempfile.mkdtemp(prefix="walt_soak_rpbat_", dir=base)
            try:
                seqs = make_genome(rng, pattern)
                fa = os.path.join(tmp, "g.fa")
                with open(fa, "w") as f:
                    for nm, s in seqs:
                        f.write(">%s\n%s\n" % (nm, s))
                path = os.path.join(tmp, "g.dbindex")
                walt_amd.makedb(fa, path, threads=4)
                db = refio.DbIndex(path)
                idx = walt_amd.Index.open(path, device=0, strands=walt_amd.STRANDS_ALL)
                try:
                    g_opt = rng.choice([0, 0, 0, 1, 2])
                    if g_opt:
                        idx.set_option("grid", g_opt)
                    lengths = [lo + 2, 40, 60, 100, 100, 131, min(150, hi), hi]
                    m, b = rng.choice([0, 2, 6, 10]), rng.choice([2, 30, 5000])
                    reads = [sample(rng, seqs, 1, rng.choice(["CT", "GA"]), lengths, refio)[0] for _ in range(1500)]
                    c, _ = refio.oracle_se(db, reads, ag=False, max_mm=m, b=b)
                    g, _ = refio.oracle_se(db, reads, ag=True, max_mm=m, b=b)
                    got, conv, _ = idx.map_se_rpbat_batch(*walt_amd.pack_reads(reads), max_mismatches=m, b=b)
                finally:
                    idx.close()
                want, want_conv = rpbat_rule(c, g)
                for f in ("genome_pos", "times", "strand", "mismatch"):
                    if not np.array_equal(got[f], want[f]):
                        bad = int(np.nonzero(got[f] != want[f])[0][0])
                        raise SoakMismatch("MISMATCH random PBAT seed %d field %s read %d (%s) m=%d b=%d" % (seed, f, bad, reads[bad], m, b))
                if not np.array_equal(conv, want_conv):
                    bad = int(np.nonzero(conv != want_conv)[0][0])
                    raise SoakMismatch("MISMATCH random PBAT seed %d conv read %d (%s) m=%d b=%d" % (seed, bad, reads[bad], m, b))
                reads_total += len(reads)
            finally:
                shutil.rmtree(tmp, ignore_errors=True)
    finally:
        refio.set_pattern(3)
        walt_amd.set_pattern(3)
    return "soak ok: random PBAT, pattern %d, %d genomes, %d reads identical to the rule on the oracle" % (
        pattern, len(seeds), reads_total)


def sample_pairs(rng, seqs, n, lengths, frag_range, refio):
    """n bisulfite pairs of either orientation: a fragment of a random strand, mate 1 its C->T converted start, mate 2
    the reverse complement of its converted end (T-rich mate first); the mates of about half of the pairs exchanged
    (A-rich mate first), and a tenth of the pairs two unrelated reads."""
    out1, out2 = [], []
    while len(out1) < n:
        l1, l2 = rng.choice(lengths), rng.choice(lengths)
        _, g = seqs[rng.randrange(len(seqs))]
        f_len = rng.randrange(max(l1, l2), max(l1, l2) + frag_range + 1)
        if rng.random() < 0.1 or len(g) < f_len:
            m1, m2 = sample(rng, seqs, 1, "CT", lengths, refio)[0], sample(rng, seqs, 1, "GA", lengths, refio)[0]
        else:
            p = rng.randrange(0, len(g) - f_len + 1)
            f = g[p:p + f_len]
            if rng.random() < 0.5:
                f = refio.revcomp(f)
            f = "".join("T" if (c == "C" and rng.random() < 0.9) else c for c in f)
            rate = rng.choice([0.0, 0.01, 0.04])
            m1, m2 = f[:l1], refio.revcomp(f[-l2:])
            m1, m2 = ("".join(rng.choice("ACGT") if rng.random() < rate else c for c in m) for m in (m1, m2))
        if rng.random() < 0.5:
            m1, m2 = m2, m1
        out1.append(m1)
        out2.append(m2)
    return out1, out2


def run_soak_pe_rpbat(seeds, pattern=3):
    """Paired-end random PBAT (walt_map_pe_rpbat_batch) on the genomes of `seeds`: pairs of either orientation, random
    m, b, k and L; the GPU's records and conversions compared with the rule of include/walt_amd.h applied to the
    oracle's two orientations (tests/test_pe_rpbat_cpu.py).  Returns the summary line, raises SoakMismatch at the first
    difference (tests/test_gpu_pe_rpbat_soak.py)."""
    import refio
    import walt_amd
    import test_pe_rpbat_cpu as rule_of
    refio.set_pattern(pattern)
    walt_amd.set_pattern(pattern)
    lo, hi = refio.MIN_READ_LEN[pattern], min(refio.MAX_READ_LEN[pattern], 260)
    base = "/dev/shm" if os.path.isdir("/dev/shm") else None
    pairs_total = 0
    rules = np.zeros(6, dtype=np.int64)
    try:
        for seed in seeds:
            rng = random.Random(seed * 7727 + 3)  # a generator of its own: run_soak's draws for a seed stay as they are
            tmp = tempfile.mkdtemp(prefix="walt_soak_pe_rpbat_", dir=base)
            try:
                seqs = make_genome(rng, pattern)
                fa = os.path.join(tmp, "g.fa")
                with open(fa, "w") as f:
                    for nm, sq in seqs:
                        f.write(">%s\n%s\n" % (nm, sq))
                path = os.path.join(tmp, "g.dbindex")
                walt_amd.makedb(fa, path, threads=4)
                db = refio.DbIndex(path)
                idx = walt_amd.Index.open(path, device=0, strands=walt_amd.STRANDS_ALL)
                m, b, k = rng.choice([0, 2, 6, 10]), rng.choice([2, 30, 5000]), rng.choice([2, 5, 50, 300])
                L = rng.choice([200, 1000])
                lengths = [lo + 2, 40, 60, 100, 100, 131, min(150, hi)]
                s1, s2 = sample_pairs(rng, seqs, 500, lengths, L, refio)
                try:
                    if rng.random() < 0.3:
                        idx.set_option("pe_chunk", 128)  # several passes: both pipeline slots
                    got, conv, _ = idx.map_pe_rpbat_batch(*walt_amd.pack_reads(s1), *walt_amd.pack_reads(s2),
                                                          max_mismatches=m, b=b, top_k=k, frag_range=L)
                finally:
                    idx.close()
                rec, want_conv, rule, _ = rule_of.oracle_pe_rpbat(db, s1, s2, m=m, b=b, k=k, L=L)
                try:
                    rule_of.compare(got, conv, rec, want_conv)
                except AssertionError as e:
                    raise SoakMismatch("MISMATCH paired-end random PBAT seed %d m=%d b=%d k=%d L=%d: %s" % (seed, m, b, k, L, e))
                rules += np.bincount(rule, minlength=6)
                pairs_total += len(s1)
            finally:
                shutil.rmtree(tmp, ignore_errors=True)
    finally:
        refio.set_pattern(3)
        walt_amd.set_pattern(3)
    return ("soak ok: paired-end random PBAT, pattern %d, %d genomes, %d pairs identical to the rule on the oracle "
            "(rules 1-5: %s)" % (pattern, len(seeds), pairs_total, list(rules[1:])))


def run_soak_meth(seeds, pattern=3):
    """Methylation calls (walt_meth_call_batch) on the genomes of `seeds`: reads of both conversions, partly
    converted, mapped on the GPU and called; calls, per-read counts and batch totals of EVERY read compared with the
    restatement of include/walt_amd.h's table in tests/test_gpu_meth.py, on an index opened with the strands of one
    conversion plus the reference and on a four-strand index through walt_index_enable_reference.  Returns the summary
    line, raises SoakMismatch at the first difference (tests/test_gpu_meth_soak.py)."""
    import refio
    import walt_amd
    import test_gpu_meth as rule_of
    refio.set_pattern(pattern)
    walt_amd.set_pattern(pattern)
    lo, hi = refio.MIN_READ_LEN[pattern], min(refio.MAX_READ_LEN[pattern], 260)
    base = "/dev/shm" if os.path.isdir("/dev/shm") else None
    reads_total = calls_total = 0
    try:
        for seed in seeds:
            rng = random.Random(seed * 15485863 + 7)  # a generator of its own: run_soak's draws for a seed stay as they are
            tmp = tempfile.mkdtemp(prefix="walt_soak_meth_", dir=base)
            try:
                seqs = make_genome(rng, pattern, many=True)
                fa = os.path.join(tmp, "g.fa")
                with open(fa, "w") as f:
                    for nm, sq in seqs:
                        f.write(">%s\n%s\n" % (nm, sq))
                path = os.path.join(tmp, "g.dbindex")
                walt_amd.makedb(fa, path, threads=4)
                db = refio.DbIndex(path)
                R = rule_of.reference_bases(db)
                lengths = [lo + 2, 40, 47, 60, 100, 100, 131, min(150, hi), hi]
                for conv, ag in (("CT", False), ("GA", True)):
                    if rng.random() < 0.5:
                        idx = walt_amd.Index.open(path, device=0, strands=(walt_amd.STRANDS_GA if ag else walt_amd.STRANDS_CT) |
                                                  walt_amd.WITH_REFERENCE)
                    else:
                        idx = walt_amd.Index.open(path, device=0, strands=walt_amd.STRANDS_ALL)
                        idx.enable_reference()
                    try:
                        reads = sample(rng, seqs, 800, conv, lengths, refio)
                        # (sample converts 90 % of the C / G: put some back, so that methylated calls are as common)
                        frm, to = ("T", "C") if conv == "CT" else ("A", "G")
                        reads = ["".join(to if (c == frm and rng.random() < 0.1) else c for c in r) for r in reads]
                        call_len = None
                        if rng.random() < 0.5:
                            call_len = [rng.choice([len(r), len(r), len(r) // 2, 0, len(r) + 3]) for r in reads]
                        bases, offs = walt_amd.pack_reads(reads)
                        recs, _ = idx.map_se_batch(bases, offs, ag_wildcard=ag, max_mismatches=rng.choice([2, 6, 10]))
                        got = idx.meth_call_batch(bases, offs, recs, "A" if ag else "T", call_len=call_len)
                    finally:
                        idx.close()
                    want = rule_of.expected_batch(db, reads, recs, "A" if ag else "T", call_len, R=R)
                    try:
                        rule_of.assert_batch(got, reads, want, "seed %d %s" % (seed, conv))
                    except AssertionError as e:
                        raise SoakMismatch("MISMATCH methylation calls seed %d %s: %s" % (seed, conv, e))
                    reads_total += len(reads)
                    calls_total += int(want[1].sum())
            finally:
                shutil.rmtree(tmp, ignore_errors=True)
    finally:
        refio.set_pattern(3)
        walt_amd.set_pattern(3)
    return "soak ok: methylation calls, pattern %d, %d genomes, %d reads (%d calls) identical to the restatement" % (
        pattern, len(seeds), reads_total, calls_total)


def run_soak_pileup(seeds, pattern=3):
    """Per-cytosine pile-up (walt_meth_pileup_batch, walt_pileup_extract) on the genomes of `seeds` (many of them with
    hundreds of short chromosomes): reads of both conversions and both strands, some with call_len, mapped on the GPU and
    piled into ONE pile-up per genome; the WHOLE extracted table compared with the restatement in
    tests/test_gpu_pileup.py, under either shape of the adds and a random extraction grid.  Returns the summary line,
    raises SoakMismatch at the first difference (tests/test_gpu_pileup_soak.py)."""
    import refio
    import walt_amd
    import test_gpu_meth as rule_of
    import test_gpu_pileup as pile_of
    refio.set_pattern(pattern)
    walt_amd.set_pattern(pattern)
    lo, hi = refio.MIN_READ_LEN[pattern], min(refio.MAX_READ_LEN[pattern], 260)
    base = "/dev/shm" if os.path.isdir("/dev/shm") else None
    reads_total = sites_total = 0
    try:
        for seed in seeds:
            rng = random.Random(seed * 32452843 + 11)
            tmp = tempfile.mkdtemp(prefix="walt_soak_pile_", dir=base)
            try:
                seqs = make_genome(rng, pattern, many=True)
                fa = os.path.join(tmp, "g.fa")
                with open(fa, "w") as f:
                    for nm, sq in seqs:
                        f.write(">%s\n%s\n" % (nm, sq))
                path = os.path.join(tmp, "g.dbindex")
                walt_amd.makedb(fa, path, threads=4)
                db = refio.DbIndex(path)
                R = rule_of.reference_bases(db)
                lengths = [lo + 2, 40, 47, 60, 100, 100, 131, min(150, hi), hi]
                idx = walt_amd.Index.open(path, device=0, strands=walt_amd.STRANDS_ALL | walt_amd.WITH_REFERENCE)
                pile = None
                try:
                    idx.set_option("pile_rows", rng.choice([0, 1]))
                    idx.set_option("pile_extract_blocks", rng.choice([0, 0, 1, 3, 64, 5000]))
                    pile = idx.pileup()
                    acc = None
                    for conv, ag in (("CT", False), ("GA", True)):
                        reads = sample(rng, seqs, 800, conv, lengths, refio)
                        frm, to = ("T", "C") if conv == "CT" else ("A", "G")
                        reads = ["".join(to if (c == frm and rng.random() < 0.1) else c for c in r) for r in reads]
                        call_len = None
                        if rng.random() < 0.5:
                            call_len = [rng.choice([len(r), len(r), len(r) // 2, 0, len(r) + 3]) for r in reads]
                        bases, offs = walt_amd.pack_reads(reads)
                        recs, _ = idx.map_se_batch(bases, offs, ag_wildcard=ag, max_mismatches=rng.choice([2, 6, 10]))
                        cv = "A" if ag else "T"
                        got = pile.add_batch(bases, offs, recs, cv, call_len=call_len)
                        plain = idx.meth_call_batch(bases, offs, recs, cv, call_len=call_len)
                        if any(g.tobytes() != p.tobytes() for g, p in zip(got, plain)):
                            raise SoakMismatch("MISMATCH pile-up seed %d %s: per-read outputs differ from meth_call_batch" % (seed, conv))
                        acc = pile_of.expected_counts(R, db.start_index, reads, recs, cv, call_len, into=acc)
                        reads_total += len(reads)
                    try:
                        sites = pile_of.assert_table(pile.extract(), R[0], db.start_index, acc[0], acc[1], "seed %d" % seed)
                    except AssertionError as e:
                        raise SoakMismatch("MISMATCH pile-up seed %d: %s" % (seed, e))
                    sites_total += int(sites.size)
                finally:
                    if pile is not None:
                        pile.close()
                    idx.close()
            finally:
                shutil.rmtree(tmp, ignore_errors=True)
    finally:
        refio.set_pattern(3)
        walt_amd.set_pattern(3)
    return "soak ok: pile-up, pattern %d, %d genomes, %d reads, %d sites identical to the restatement" % (
        pattern, len(seeds), reads_total, sites_total)


def run_soak_dedup(seeds, pattern=3):
    """Duplicate marking (walt_dedup_*, walt_meth_pileup_batch_skip) on the genomes of `seeds`: single-end reads of either
    conversion and pairs of either orientation, sampled WITH replacement so that about a third are copies of earlier
    ones; mapped on the GPU (random-PBAT calls), fed to a set that starts at 64 slots in calls cut at random points, and
    the verdicts compared with the restatement in tests/test_dedup_cpu.py; the pile-up of the records that are no
    duplicates compared with the restatement in tests/test_gpu_pileup.py.  Returns the summary line, raises SoakMismatch
    at the first difference (tests/test_gpu_dedup.py)."""
    import refio
    import walt_amd
    import test_dedup_cpu as rule_of
    import test_gpu_meth as meth_of
    import test_gpu_pileup as pile_of
    refio.set_pattern(pattern)
    walt_amd.set_pattern(pattern)
    lo, hi = refio.MIN_READ_LEN[pattern], min(refio.MAX_READ_LEN[pattern], 160)
    base = "/dev/shm" if os.path.isdir("/dev/shm") else None
    reads_total = dups_total = 0
    try:
        for seed in seeds:
            rng = random.Random(seed * 15485863 + 5)
            tmp = tempfile.mkdtemp(prefix="walt_soak_dedup_", dir=base)
            try:
                seqs = make_genome(rng, pattern)
                fa = os.path.join(tmp, "g.fa")
                with open(fa, "w") as f:
                    for nm, sq in seqs:
                        f.write(">%s\n%s\n" % (nm, sq))
                path = os.path.join(tmp, "g.dbindex")
                walt_amd.makedb(fa, path, threads=4)
                db = refio.DbIndex(path)
                R = meth_of.reference_bases(db)
                lengths = [lo + 2, 47, 60, 100, 100, min(150, hi)]
                idx = walt_amd.Index.open(path, device=0, strands=walt_amd.STRANDS_ALL | walt_amd.WITH_REFERENCE)
                dd = pile = None
                try:
                    dd = walt_amd.Dedup(initial_slots=64, pattern=pattern)
                    pile = idx.pileup()
                    rule = rule_of.DupRule()
                    acc = None
                    # single-end: 400 distinct reads of either conversion, 600 drawn from them with replacement
                    distinct = sample(rng, seqs, 200, "CT", lengths, refio) + sample(rng, seqs, 200, "GA", lengths, refio)
                    reads = [rng.choice(distinct) for _ in range(600)]
                    bases, offs = walt_amd.pack_reads(reads)
                    recs, conv, _ = idx.map_se_rpbat_batch(bases, offs)
                    got, at = [], 0
                    while at < len(reads):
                        n = rng.choice([1, 7, 64, 65, 300])
                        got.append(dd.add_batch(recs[at:at + n], conv[at:at + n]))
                        at += n
                    got = np.concatenate(got)
                    want = rule_of.expect_single(rule, recs, conv)
                    if got.tolist() != want.tolist():
                        raise SoakMismatch("MISMATCH dedup seed %d: single-end verdicts differ at %s" % (
                            seed, np.nonzero(got != want)[0][:5].tolist()))
                    pile.add_batch(bases, offs, recs, conv, skip=got, want_calls=False, want_counts=False, want_stats=False)
                    kept = recs.copy()
                    kept["times"][got != 0] = 0
                    acc = pile_of.expected_counts(R, db.start_index, reads, kept, conv, into=acc)
                    reads_total += len(reads)
                    dups_total += int(got.sum())
                    # pairs: the same set goes on (lone mates have kinds of their own)
                    d1, d2 = sample_pairs(rng, seqs, 300, lengths, 400, refio)
                    pick = [rng.randrange(len(d1)) for _ in range(450)]
                    r1, r2 = [d1[i] for i in pick], [d2[i] for i in pick]
                    b1, o1 = walt_amd.pack_reads(r1)
                    b2, o2 = walt_amd.pack_reads(r2)
                    res, pconv, _ = idx.map_pe_rpbat_batch(b1, o1, b2, o2, frag_range=400 + hi)
                    gotp, at = [], 0
                    while at < len(r1):
                        n = rng.choice([1, 7, 64, 200])
                        gotp.append(dd.add_pairs(res[at:at + n], pconv[at:at + n]))
                        at += n
                    gotp = np.concatenate(gotp)
                    wantp = rule_of.expect_pairs(rule, res, pconv)
                    if gotp.tolist() != wantp.tolist():
                        raise SoakMismatch("MISMATCH dedup seed %d: paired-end verdicts differ at %s" % (
                            seed, np.nonzero((gotp != wantp).any(axis=1))[0][:5].tolist()))
                    if dd.count() != (len(rule.first), rule.fed):
                        raise SoakMismatch("MISMATCH dedup seed %d: count %s against %s" % (seed, dd.count(), (len(rule.first), rule.fed)))
                    for k, (rd, b, o) in enumerate(((r1, b1, o1), (r2, b2, o2))):
                        m = res["m%d" % (k + 1)]
                        pile.add_batch(b, o, m, pconv[:, k], skip=gotp[:, k], want_calls=False, want_counts=False, want_stats=False)
                        kept = np.ascontiguousarray(m).copy()
                        kept["times"][gotp[:, k] != 0] = 0
                        acc = pile_of.expected_counts(R, db.start_index, rd, kept, pconv[:, k], into=acc)
                    reads_total += 2 * len(r1)
                    dups_total += int(gotp.sum())
                    try:
                        pile_of.assert_table(pile.extract(), R[0], db.start_index, acc[0], acc[1], "seed %d" % seed)
                    except AssertionError as e:
                        raise SoakMismatch("MISMATCH dedup seed %d: %s" % (seed, e))
                finally:
                    if pile is not None:
                        pile.close()
                    if dd is not None:
                        dd.close()
                    idx.close()
            finally:
                shutil.rmtree(tmp, ignore_errors=True)
    finally:
        refio.set_pattern(3)
        walt_amd.set_pattern(3)
    if dups_total * 5 < reads_total:
        raise SoakMismatch("soak too thin: %d duplicates among %d reads" % (dups_total, reads_total))
    return "soak ok: duplicates, pattern %d, %d genomes, %d reads, %d duplicates identical to the restatement" % (
        pattern, len(seeds), reads_total, dups_total)


def sample_fragments(rng, seqs, n, lo, hi, refio):
    """n bisulfite pairs cut from fragments of lo + 2 bases (shorter than one read: the mates are the whole fragment) up
    to 2 hi + 120 (longer than two reads: no overlap): mate 1 the fragment's C->T converted start, mate 2 the reverse
    complement of its end, about half of the C kept; a tenth of the pairs two unrelated reads."""
    out1, out2 = [], []
    while len(out1) < n:
        _, g = seqs[rng.randrange(len(seqs))]
        f_len = rng.choice([lo + 2, rng.randrange(lo + 2, hi + 1), rng.randrange(hi, 2 * hi + 1), rng.randrange(2 * hi, 2 * hi + 121)])
        if rng.random() < 0.1:
            out1.append(sample(rng, seqs, 1, "CT", [lo + 2, 60, 100], refio)[0])
            out2.append(sample(rng, seqs, 1, "GA", [lo + 2, 60, 100], refio)[0])
            continue
        if len(g) < f_len:
            continue
        p = rng.randrange(0, len(g) - f_len + 1)
        if rng.random() < 0.3:
            p = rng.choice([0, len(g) - f_len])
        f = g[p:p + f_len]
        if rng.random() < 0.5:
            f = refio.revcomp(f)
        f = "".join("T" if (c == "C" and rng.random() < 0.5) else c for c in f)
        l1, l2 = (min(f_len, rng.choice([lo + 2, 60, 100, hi])) for _ in range(2))
        out1.append(f[:l1])
        out2.append(refio.revcomp(f[-l2:]))
    return out1, out2


def run_soak_overlap(seeds, pattern=3):
    """The overlap of a pair (walt_pair_overlap_batch, walt_meth_pileup_batch_excl) on the genomes of `seeds` (many of
    them with hundreds of short chromosomes): pairs cut from fragments shorter than one read up to longer than two, some
    with call_len on either mate, mapped on the GPU; the interval words, the totals, both mates' calls, counts and batch
    totals and the WHOLE table of the one pile-up both mates go into compared with the brute-force restatement in
    tests/test_gpu_overlap.py, under either shape of the adds.  Returns the summary line, raises SoakMismatch at the
    first difference (tests/test_gpu_overlap.py)."""
    import refio
    import walt_amd
    import test_gpu_meth as meth_of
    import test_gpu_overlap as rule_of
    refio.set_pattern(pattern)
    walt_amd.set_pattern(pattern)
    lo, hi = refio.MIN_READ_LEN[pattern], min(refio.MAX_READ_LEN[pattern], 150)
    base = "/dev/shm" if os.path.isdir("/dev/shm") else None
    pairs_total = overlap_total = bases_total = 0
    try:
        for seed in seeds:
            rng = random.Random(seed * 49979687 + 13)
            tmp = tempfile.mkdtemp(prefix="walt_soak_overlap_", dir=base)
            try:
                seqs = make_genome(rng, pattern, many=True)
                fa = os.path.join(tmp, "g.fa")
                with open(fa, "w") as f:
                    for nm, sq in seqs:
                        f.write(">%s\n%s\n" % (nm, sq))
                path = os.path.join(tmp, "g.dbindex")
                walt_amd.makedb(fa, path, threads=4)
                db = refio.DbIndex(path)
                R = meth_of.reference_bases(db)
                idx = walt_amd.Index.open(path, device=0, strands=walt_amd.STRANDS_ALL | walt_amd.WITH_REFERENCE)
                try:
                    idx.set_option("pile_rows", rng.choice([0, 1]))
                    r1, r2 = sample_fragments(rng, seqs, 400, lo, hi, refio)
                    b1, o1 = walt_amd.pack_reads(r1)
                    b2, o2 = walt_amd.pack_reads(r2)
                    res, _ = idx.map_pe_batch(b1, o1, b2, o2, frag_range=2 * hi + 200)
                    cl1 = cl2 = None
                    if rng.random() < 0.5:
                        cl1 = [rng.choice([len(r), len(r), len(r) // 2, 0, 1, len(r) + 3]) for r in r1]
                    if rng.random() < 0.5:
                        cl2 = [rng.choice([len(r), len(r), len(r) // 2, 0, 1, len(r) + 3]) for r in r2]
                    try:
                        want, _ = rule_of.run_pairs(idx, R, db.start_index, r1, r2, res, "T", "A", cl1, cl2, what="seed %d" % seed)
                    except AssertionError as e:
                        raise SoakMismatch("MISMATCH overlap seed %d: %s" % (seed, e))
                    pairs_total += len(r1)
                    overlap_total += want["totals"][0]
                    bases_total += want["totals"][1]
                finally:
                    idx.close()
            finally:
                shutil.rmtree(tmp, ignore_errors=True)
    finally:
        refio.set_pattern(3)
        walt_amd.set_pattern(3)
    if overlap_total * 10 < pairs_total:
        raise SoakMismatch("soak too thin: %d overlapping pairs among %d" % (overlap_total, pairs_total))
    return "soak ok: overlap, pattern %d, %d genomes, %d pairs, %d with an overlap (%d mate-2 bases) identical to the restatement" % (
        pattern, len(seeds), pairs_total, overlap_total, bases_total)


def run_soak_mbias(seeds, pattern=3):
    """Methylation bias by read position (walt_mbias_*, walt_meth_pileup_batch_mbias) on the genomes of `seeds`: pairs cut
    from fragments of every length, some with call_len, skip bytes and the excluded intervals of their overlap, mapped
    and called on the GPU with one table per mate; each table compared with the restatement in tests/test_gpu_mbias.py
    over the calls that came back, its column sums with the batch totals, and the same calls fed again through
    walt_mbias_batch double every count.  Returns the summary line, raises SoakMismatch at the first difference."""
    import refio
    import walt_amd
    import test_gpu_mbias as rule_of
    refio.set_pattern(pattern)
    walt_amd.set_pattern(pattern)
    lo, hi = refio.MIN_READ_LEN[pattern], min(refio.MAX_READ_LEN[pattern], 150)
    base = "/dev/shm" if os.path.isdir("/dev/shm") else None
    pairs_total = calls_total = 0
    mb = walt_amd.MBias(0, 2, pattern=pattern)
    try:
        for seed in seeds:
            rng = random.Random(seed * 86028121 + 19)
            tmp = tempfile.mkdtemp(prefix="walt_soak_mbias_", dir=base)
            try:
                seqs = make_genome(rng, pattern, many=rng.random() < 0.3)
                fa = os.path.join(tmp, "g.fa")
                with open(fa, "w") as f:
                    for nm, sq in seqs:
                        f.write(">%s\n%s\n" % (nm, sq))
                path = os.path.join(tmp, "g.dbindex")
                walt_amd.makedb(fa, path, threads=4)
                idx = walt_amd.Index.open(path, device=0, strands=walt_amd.STRANDS_ALL | walt_amd.WITH_REFERENCE)
                try:
                    r1, r2 = sample_fragments(rng, seqs, 300, lo, hi, refio)
                    b1, o1 = walt_amd.pack_reads(r1)
                    b2, o2 = walt_amd.pack_reads(r2)
                    res, _ = idx.map_pe_batch(b1, o1, b2, o2, frag_range=2 * hi + 200)
                    excl, _ = idx.pair_overlap(res, o1, o2)
                    mb.clear()
                    for k, (b, o, reads, mate, cv) in enumerate(((b1, o1, r1, "m1", "T"), (b2, o2, r2, "m2", "A"))):
                        cl = [rng.choice([len(r), len(r), len(r) // 2, 0, len(r) + 3]) for r in reads] if rng.random() < 0.5 else None
                        skip = np.array([rng.random() < 0.2 for _ in reads], dtype=np.uint8) if rng.random() < 0.5 else None
                        ex = excl if k == 1 and rng.random() < 0.7 else None
                        calls, _, stats = idx.meth_call_batch(b, o, res[mate], cv, call_len=cl, skip=skip, excl=ex, mbias=mb, mbias_table=k)
                        want = rule_of.expected_table(calls, o, res[mate]["times"], skip)
                        got = mb.read(k)
                        if not np.array_equal(got, want):
                            raise SoakMismatch("MISMATCH mbias seed %d mate %d: table differs at %s" % (seed, k + 1, np.argwhere(got != want)[:4].tolist()))
                        m, u = rule_of.column_sums(got)
                        if not (np.array_equal(m, stats["meth"][0]) and np.array_equal(u, stats["unmeth"][0])):
                            raise SoakMismatch("MISMATCH mbias seed %d mate %d: column sums %s %s, totals %s" % (seed, k + 1, m, u, stats))
                        mb.add(calls, o, res[mate], skip=skip, table=k)
                        if not np.array_equal(mb.read(k), want * np.uint64(2)):
                            raise SoakMismatch("MISMATCH mbias seed %d mate %d: the same calls fed again do not double the table" % (seed, k + 1))
                        calls_total += int(want.sum())
                    pairs_total += len(r1)
                finally:
                    idx.close()
            finally:
                shutil.rmtree(tmp, ignore_errors=True)
    finally:
        mb.close()
        refio.set_pattern(3)
        walt_amd.set_pattern(3)
    if calls_total < 10 * pairs_total:
        raise SoakMismatch("soak too thin: %d calls counted over %d pairs" % (calls_total, pairs_total))
    return "soak ok: mbias, pattern %d, %d genomes, %d pairs, %d calls counted by read position identical to the restatement" % (
        pattern, len(seeds), pairs_total, calls_total)


def run_soak_nonconv(seeds, pattern=3):
    """Non-converted reads (walt_meth_nonconv_batch, walt_nonconv_batch, walt_nonconv_pairs_batch) on the genomes of `seeds`:
    pairs cut from fragments of every length, some with call_len, mapped on the GPU; each mate called and judged in one
    step under a random rule, the verdicts and tallies compared with the restatement in tests/test_gpu_nonconv.py over the
    calls of the plain calling call, the pair rule with its restatement, and the totals of the calling call that takes the
    verdicts as skip bytes with the letters of the kept unique records counted in Python.  Returns the summary line, raises
    SoakMismatch at the first difference."""
    import refio
    import walt_amd
    import test_gpu_nonconv as rule_of
    refio.set_pattern(pattern)
    walt_amd.set_pattern(pattern)
    lo, hi = refio.MIN_READ_LEN[pattern], min(refio.MAX_READ_LEN[pattern], 150)
    base = "/dev/shm" if os.path.isdir("/dev/shm") else None
    pairs_total = judged_total = filtered_total = 0
    try:
        for seed in seeds:
            rng = random.Random(seed * 49979687 + 23)
            tmp = tempfile.mkdtemp(prefix="walt_soak_nonconv_", dir=base)
            try:
                seqs = make_genome(rng, pattern, many=rng.random() < 0.3)
                fa = os.path.join(tmp, "g.fa")
                with open(fa, "w") as f:
                    for nm, sq in seqs:
                        f.write(">%s\n%s\n" % (nm, sq))
                path = os.path.join(tmp, "g.dbindex")
                walt_amd.makedb(fa, path, threads=4)
                idx = walt_amd.Index.open(path, device=0, strands=walt_amd.STRANDS_ALL | walt_amd.WITH_REFERENCE)
                try:
                    r1, r2 = sample_fragments(rng, seqs, 300, lo, hi, refio)
                    b1, o1 = walt_amd.pack_reads(r1)
                    b2, o2 = walt_amd.pack_reads(r2)
                    res, _ = idx.map_pe_batch(b1, o1, b2, o2, frag_range=2 * hi + 200)
                    # (the library keeps about half of its C: rules around that level, so that both outcomes occur)
                    rule = (rng.choice([0, 0, 8, 12, 20]), rng.choice([0, 0, 4, 6]), rng.choice([0, 0, 50, 60, 100]), rng.choice([0, 1, 5, 12]))
                    if not any(rule[:3]):
                        rule = (10,) + rule[1:]
                    r = walt_amd.nonconv_rule(*rule)
                    cols, kept = [], []
                    for k, (b, o, reads, mate, cv) in enumerate(((b1, o1, r1, "m1", "T"), (b2, o2, r2, "m2", "A"))):
                        cl = [rng.choice([len(x), len(x), len(x) // 2, 0, len(x) + 3]) for x in reads] if rng.random() < 0.5 else None
                        calls = idx.meth_call_batch(b, o, res[mate], cv, call_len=cl, want_counts=False, want_stats=False)[0]
                        want_f, want_t = rule_of.expected_verdicts(calls, o, res[mate]["times"], rule)
                        filt, tally, got_calls = idx.meth_nonconv_batch(b, o, res[mate], r, cv, call_len=cl, want_calls=True)
                        again, tally2 = idx.nonconv_batch(calls, o, res[mate], r)
                        if got_calls.tobytes() != calls.tobytes():
                            raise SoakMismatch("MISMATCH nonconv seed %d mate %d: the calls of the one-step form differ" % (seed, k + 1))
                        for f, t in ((filt, tally), (again, tally2)):
                            if not (np.array_equal(f, want_f) and np.array_equal(rule_of.tally_array(t), want_t)):
                                bad = np.nonzero((f != want_f) | (rule_of.tally_array(t) != want_t).any(axis=1))[0][:4]
                                raise SoakMismatch("MISMATCH nonconv seed %d mate %d rule %s: reads %s" % (seed, k + 1, rule, bad.tolist()))
                        cols.append(filt)
                        kept.append((b, o, mate, cv, cl, calls))
                        judged_total += int((res[mate]["times"] == 1).sum())
                    filt = np.stack(cols, axis=1)
                    want = rule_of.pair_rule(filt, res["best_times"])
                    got = idx.nonconv_pairs(res, filt.copy())
                    if not np.array_equal(got, want):
                        raise SoakMismatch("MISMATCH nonconv seed %d: the pair rule differs at %s" % (seed, np.argwhere(got != want)[:4].tolist()))
                    for k, (b, o, mate, cv, cl, calls) in enumerate(kept):
                        stats = idx.meth_call_batch(b, o, res[mate], cv, call_len=cl, want_calls=False, want_counts=False,
                                                    skip=np.ascontiguousarray(got[:, k]))[2]
                        m, u, reads = np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.uint64), 0
                        for i in range(len(o) - 1):
                            if int(res[mate]["times"][i]) != 1 or got[i, k]:
                                continue
                            reads += 1
                            seg = calls[int(o[i]):int(o[i + 1])].tobytes()
                            for c, pair in enumerate(("zZ", "xX", "hH", "uU")):
                                u[c] += np.uint64(seg.count(pair[0].encode()))
                                m[c] += np.uint64(seg.count(pair[1].encode()))
                        if not (int(stats["reads"][0]) == reads and np.array_equal(m, stats["meth"][0]) and np.array_equal(u, stats["unmeth"][0])):
                            raise SoakMismatch("MISMATCH nonconv seed %d mate %d: totals of the filtered call %s, counted %d %s %s" % (
                                seed, k + 1, stats, reads, m, u))
                    filtered_total += int(got.sum())
                    pairs_total += len(r1)
                finally:
                    idx.close()
            finally:
                shutil.rmtree(tmp, ignore_errors=True)
    finally:
        refio.set_pattern(3)
        walt_amd.set_pattern(3)
    if filtered_total == 0 or filtered_total >= judged_total:
        raise SoakMismatch("soak too thin: %d of %d judged reads filtered" % (filtered_total, judged_total))
    return "soak ok: nonconv, pattern %d, %d genomes, %d pairs, %d unique reads judged, %d verdicts of 1, all identical to the restatement" % (
        pattern, len(seeds), pairs_total, judged_total, filtered_total)


def run_soak_trim(seeds, pattern=3):
    """Ignored read ends (walt_meth_pileup_batch_trim, walt_pair_overlap_batch_trim) on the genomes of `seeds`: pairs cut
    from fragments of every length, mapped on the GPU, then called with random bounds per mate -- 0, small, around the read
    length, beyond it -- with and without the overlap's interval, clip points, skip bytes and the pile_rows option, into a
    pile-up and a bias set.  Intervals, calls, counts, totals, the pile-up and the bias table are compared with the
    restatement of tests/test_gpu_trim.py.  Returns the summary line, raises SoakMismatch at the first difference."""
    import refio
    import walt_amd
    import test_gpu_trim as rule_of
    from test_gpu_meth import reference_bases
    from test_gpu_overlap import pile_letters
    from test_gpu_pileup import expected_table
    refio.set_pattern(pattern)
    walt_amd.set_pattern(pattern)
    lo, hi = refio.MIN_READ_LEN[pattern], min(refio.MAX_READ_LEN[pattern], 150)
    base = "/dev/shm" if os.path.isdir("/dev/shm") else None
    pairs_total = blanked_total = kept_total = 0
    mb = walt_amd.MBias(0, 2, pattern=pattern)
    try:
        for seed in seeds:
            rng = random.Random(seed * 49979687 + 23)
            tmp = tempfile.mkdtemp(prefix="walt_soak_trim_", dir=base)
            try:
                seqs = make_genome(rng, pattern, many=rng.random() < 0.3)
                fa = os.path.join(tmp, "g.fa")
                with open(fa, "w") as f:
                    for nm, sq in seqs:
                        f.write(">%s\n%s\n" % (nm, sq))
                path = os.path.join(tmp, "g.dbindex")
                walt_amd.makedb(fa, path, threads=4)
                db = refio.DbIndex(path)
                R = reference_bases(db)
                idx = walt_amd.Index.open(path, device=0, strands=walt_amd.STRANDS_ALL | walt_amd.WITH_REFERENCE)
                pile = None
                try:
                    idx.set_option("pile_rows", rng.randrange(2))
                    r1, r2 = sample_fragments(rng, seqs, 120, lo, hi, refio)
                    b1, o1 = walt_amd.pack_reads(r1)
                    b2, o2 = walt_amd.pack_reads(r2)
                    res, _ = idx.map_pe_batch(b1, o1, b2, o2, frag_range=2 * hi + 200)
                    bound = lambda: rng.choice([0, 0, rng.randrange(1, 20), rng.randrange(lo - 3, hi + 3), 5000])
                    t = [(bound(), bound()), (bound(), bound())]
                    cl = [[rng.choice([len(r), len(r), len(r) // 2, 0, len(r) + 3]) for r in reads] if rng.random() < 0.5 else None
                          for reads in (r1, r2)]
                    skip = np.array([[rng.random() < 0.2, rng.random() < 0.2] for _ in r1], dtype=np.uint8) if rng.random() < 0.5 else None
                    no_overlap = rng.random() < 0.6
                    ex = words = None
                    if no_overlap:
                        ex, words, totals = rule_of.want_words(db.start_index, db.genome_len, res, r1, r2, cl[0], cl[1], t[0], t[1])
                        got_words, got_totals = idx.pair_overlap(res, o1, o2, cl[0], cl[1], trim1=t[0], trim2=t[1])
                        if got_words.tolist() != words.tolist() or got_totals.tolist() != totals:
                            raise SoakMismatch("MISMATCH trim seed %d: intervals or totals differ under bounds %s (%s against %s)" % (
                                seed, t, got_totals.tolist(), totals))
                    pile = idx.pileup()
                    mb.clear()
                    acc = None
                    for k, (b, o, reads, mate, cv) in enumerate(((b1, o1, r1, "m1", "T"), (b2, o2, r2, "m2", "A"))):
                        sk = None if skip is None else skip[:, k]
                        want = rule_of.want_mate(R, db.start_index, reads, res[mate], cv, cl[k], ex if k else None, sk, t[k])
                        got = pile.add_batch(b, o, res[mate], cv, call_len=cl[k], skip=sk, excl=words if k else None, mbias=mb, mbias_table=k,
                                             trim5=t[k][0], trim3=t[k][1])
                        try:
                            rule_of.assert_mate(got, want, "seed %d mate %d bounds %s" % (seed, k + 1, t[k]))
                        except AssertionError as e:
                            raise SoakMismatch("MISMATCH trim " + str(e)[:600])
                        if not np.array_equal(mb.read(k), rule_of.want_table(want[0], o, res[mate], sk)):
                            raise SoakMismatch("MISMATCH trim seed %d mate %d: the bias table differs" % (seed, k + 1))
                        acc = pile_letters(db.start_index, db.genome_len, want[0], res[mate], sk, into=acc)
                        plain = rule_of.want_mate(R, db.start_index, reads, res[mate], cv, cl[k], ex if k else None, sk)
                        kept_total += int(want[1].sum())
                        blanked_total += int(plain[1].sum() - want[1].sum())
                    sites, off = pile.extract()
                    want_sites, want_off = expected_table(R[0], db.start_index, *acc)
                    if sites.tobytes() != want_sites.tobytes() or [int(off[0]), int(off[1])] != want_off:
                        raise SoakMismatch("MISMATCH trim seed %d: the pile-up differs under bounds %s" % (seed, t))
                    pairs_total += len(r1)
                finally:
                    if pile is not None:
                        pile.close()
                    idx.close()
            finally:
                shutil.rmtree(tmp, ignore_errors=True)
    finally:
        mb.close()
        refio.set_pattern(3)
        walt_amd.set_pattern(3)
    if len(seeds) >= 5 and (blanked_total < pairs_total or kept_total < pairs_total):
        raise SoakMismatch("soak too thin: %d calls blanked, %d kept over %d pairs" % (blanked_total, kept_total, pairs_total))
    return "soak ok: trim, pattern %d, %d genomes, %d pairs, %d calls kept and %d ignored identical to the restatement" % (
        pattern, len(seeds), pairs_total, kept_total, blanked_total)


def rpbat_rule(c, g):
    """The random-PBAT rule (include/walt_amd.h) on two single-conversion record arrays -> (records, conv)."""
    ct, gt = c["times"].astype(np.int64), g["times"].astype(np.int64)
    r1 = (ct == 1) & (gt == 1) & (c["genome_pos"] == g["genome_pos"]) & (c["strand"] == g["strand"])
    r2 = ~r1 & ((gt == 0) | ((ct > 0) & (c["mismatch"] < g["mismatch"])))
    r3 = ~r1 & ~r2 & ((ct == 0) | (g["mismatch"] < c["mismatch"]))
    r4 = ~r1 & ~r2 & ~r3
    rec = c.copy()
    for f in ("genome_pos", "times", "strand", "mismatch"):
        rec[f] = np.where(r3, g[f], c[f])
    rec["times"][r4] = (ct + gt)[r4]
    return rec, np.where(r3, ord("A"), ord("T")).astype(np.uint8)


if __name__ == "__main__":
    main()
