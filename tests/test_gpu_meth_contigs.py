"""Methylation calls and pile-up (walt_meth_call_batch, walt_meth_pileup_batch, walt_pileup_extract*, bin/walt -M -MC)
on genomes of many sequences and on a genome larger than one window of the <out>.methcounts writer.

A record's chromosome bounds [lo, hi) decide whether a position gets a call, the u / U contexts at chromosome ends and
the forward position of a '-' record; the kernels take them from the look-up of walt_amd/csrc/chrom_core.h, which has
one path per range of sequence counts (tests/test_chrom_cpu.py runs the look-up itself on the CPU).  Here every path is
reached from the calls: 1,023 sequences (every start staged), 1,024 / 2,047 / 4,092 (five neighbouring words),
4,093 / 8,185 (a second bisection), with records at both ends of EVERY chromosome, on both strands and under both
conversions.  The larger genome takes the command line's writer through two windows and the extraction through more
than 1,024 blocks; the depth test piles tens of thousands of calls onto single counters.

Expected values come from the restatements of tests/test_gpu_meth.py and tests/test_gpu_pileup.py alone.  What makes a
case hard (which chromosomes carry records, which letters occur, where a read is cut at its chromosome's end) is
asserted from the inputs and the restatement, so a test cannot pass by leaving those cases out."""
import os
import random

import numpy as np
import pytest

import refio
from test_gpu_meth import assert_batch, cli_records_se, expected_batch, expected_read, reference_bases, run_walt, strip_xm
from test_gpu_pileup import (assert_sums_equal_stats, assert_table, counts_text, expected_counts, expected_table)

pytestmark = pytest.mark.gpu

K_LDS = 1023             # chrom_core.h kLdsChroms
COUNTS = [1023, 1024, 2047, 4092, 4093, 8185]
RANGE_COUNTS = [1023, 1024, 2047, 4093, 8185]  # one genome per shift value 0 .. 4
WINDOW = 1 << 22         # host/walt_main.cpp kCountsWindow
KINDS = ("first", "last", "over")


def shift_of(n):
    sh = 0
    while -(-n // (1 << sh)) > K_LDS:
        sh += 1
    return sh


class Genome:
    """an N-free genome: the '+' text, the '-' text (every chromosome reverse-complemented in place), the starts"""

    def __init__(self, names, seqs):
        self.names, self.seqs = names, seqs
        self.text = "".join(seqs)
        self.minus = "".join(refio.revcomp(s) for s in seqs)
        self.start_index = np.zeros(len(seqs) + 1, dtype=np.uint32)
        self.start_index[1:] = np.cumsum([len(s) for s in seqs])
        self.n_chrom, self.genome_len = len(seqs), len(self.text)
        self.R = [np.frombuffer(self.text.encode(), dtype=np.uint8), np.frombuffer(self.minus.encode(), dtype=np.uint8)]

    def write(self, fa):
        with open(fa, "w") as f:
            for nm, s in zip(self.names, self.seqs):
                f.write(">%s\n%s\n" % (nm, s))


def contig_genome(n_chrom):
    """Sequences of tens of bases, a few hundred in every 16th (long enough for reads that map), and the shortest the
    builder accepts (1, 2 and 3 bases) among them; the last one is a single base where n_chrom is odd.  C / G rich."""
    rng = random.Random(7000 + n_chrom)
    seqs = []
    for i in range(n_chrom):
        L = rng.randrange(20, 90)
        if i % 16 == 9:
            L = rng.randrange(150, 320)
        if i % 37 in (5, 11, 23):
            L = {5: 1, 11: 2, 23: 3}[i % 37]
        if i == n_chrom - 1 and n_chrom % 2:
            L = 1
        seqs.append("".join(rng.choice("ACGTCG") for _ in range(L)))
    return Genome(["s%d" % i for i in range(n_chrom)], seqs)


def cut_read(rng, G, pos, n, conv):
    """the strand genome's bases [pos, pos + n) (A beyond the genome's end), partly converted, a few mismatches"""
    s = list(G[pos:pos + n])
    s += ["A"] * (n - len(s))
    frm, to = ("C", "T") if conv == "T" else ("G", "A")
    for i, ch in enumerate(s):
        if ch == frm and rng.random() < 0.5:
            s[i] = to
        elif rng.random() < 0.03:
            s[i] = rng.choice("ACGT")
    return "".join(s)


def made_up_records(g, seed):
    """For every chromosome, strand and conversion three records with times == 1: starting at the chromosome's first
    base, ending at its last base, overhanging its end by part of the read.  Then a minority of copies with times 0,
    times 2 and a position at or beyond the genome's end.  -> (seqs, records, conv uint8, meta) where meta[i] =
    (chromosome, strand, conversion, kind) for the first 12 * n_chrom records."""
    import walt_amd
    rng = random.Random(seed)
    seqs, rows, meta = [], [], []
    for c in range(g.n_chrom):
        lo, hi = int(g.start_index[c]), int(g.start_index[c + 1])
        L = hi - lo
        for strand in (b"+", b"-"):
            G = g.minus if strand == b"-" else g.text
            for conv in "TA":
                n = min(L, rng.choice([1, 2, 3, 5, 8, 13, 17, 24, 31, L]))
                seqs.append(cut_read(rng, G, lo, n, conv))
                rows.append((lo, 1, strand, ord(conv)))
                n = min(L, rng.choice([1, 2, 3, 5, 8, 13, 17, 24, 33, L]))
                seqs.append(cut_read(rng, G, hi - n, n, conv))
                rows.append((hi - n, 1, strand, ord(conv)))
                k = rng.randrange(1, min(L, 12) + 1)  # bases inside the chromosome
                extra = rng.choice([1, 2, 5, 17, 33]) if rng.random() < 0.985 else rng.randrange(120, 290)
                seqs.append(cut_read(rng, G, hi - k, k + extra, conv))
                rows.append((hi - k, 1, strand, ord(conv)))
                meta += [(c, strand, conv, kind) for kind in KINDS]
    base = len(rows)
    for what in ("times0", "times2", "beyond"):
        for _ in range(max(30, base // 40)):
            j = rng.randrange(base)
            pos, _, strand, cv = rows[j]
            seqs.append(seqs[j])
            if what == "beyond":
                rows.append((rng.choice([g.genome_len, g.genome_len + 1, g.genome_len + 4097, 0xFFFFFFFF]), 1, strand, cv))
            else:
                rows.append((pos, 0 if what == "times0" else 2, strand, cv))
    recs = np.zeros(len(rows), dtype=walt_amd.best_match_dtype)
    recs["genome_pos"] = [r[0] for r in rows]
    recs["times"] = [r[1] for r in rows]
    recs["strand"] = [r[2] for r in rows]
    conv = np.array([r[3] for r in rows], dtype=np.uint8)
    return seqs, recs, conv, meta


def assert_coverage(g, seqs, recs, conv, meta, calls):
    """the hard cases are present -- from the records and the restatement's calls (of the made-up records) alone"""
    n, sh = g.n_chrom, shift_of(g.n_chrom)
    start = g.start_index
    # no record is skipped: every chromosome has all twelve, each a times == 1 record inside that chromosome
    assert len(meta) == 12 * n and len(set(meta)) == 12 * n and len(seqs) == len(recs) == len(conv) == len(calls)
    chrom = np.searchsorted(start, recs["genome_pos"][:len(meta)], "right") - 1
    assert np.array_equal(chrom, [m[0] for m in meta]) and (recs["times"][:len(meta)] == 1).all()
    for kind_i, kind in enumerate(KINDS):
        sel = np.arange(kind_i, len(meta), 3)
        pos, ln = recs["genome_pos"][sel].astype(np.int64), np.array([len(seqs[i]) for i in sel])
        lo, hi = start[chrom[sel]].astype(np.int64), start[chrom[sel] + 1].astype(np.int64)
        assert {"first": (pos == lo) & (pos + ln <= hi), "last": (pos + ln == hi) & (pos >= lo),
                "over": (pos < hi) & (pos + ln > hi) & (pos >= lo)}[kind].all(), kind
    # the minority: unmapped, ambiguous and made-up positions; lengths of every alignment and of more than one trip
    assert (recs["times"] == 0).sum() >= 30 and (recs["times"] == 2).sum() >= 30
    assert (recs["genome_pos"].astype(np.int64) >= g.genome_len).sum() >= 30 and int(recs["genome_pos"].max()) == 0xFFFFFFFF
    lens = np.array([len(s) for s in seqs])
    assert len(set((np.cumsum(lens) % 16).tolist())) == 16 and (lens > 128).sum() >= 20 and (lens == 1).sum() >= 20
    # which chromosomes: first and last of a sample interval, the final (partial) interval, the last chromosome
    have = set(chrom.tolist())
    m = -(-n // (1 << sh))
    assert {c for c in range(n) if c % (1 << sh) == 0} <= have and {c for c in range(n) if c % (1 << sh) == (1 << sh) - 1} <= have
    assert set(range((m - 1) << sh, n)) <= have and n - 1 in have
    if n in (2047, 4093, 8185):
        assert n % (1 << sh), "these genomes end in a partial interval"
    # the letters
    assert set("zZxXhHuU") <= set("".join(calls[:len(meta)])), set("".join(calls[:len(meta)]))
    unknown = {(m_[1], m_[2]) for m_, c in zip(meta, calls) if "u" in c or "U" in c}
    assert unknown == {(b"+", "T"), (b"+", "A"), (b"-", "T"), (b"-", "A")}, unknown
    # overhanging reads cut at hi: nothing is called from hi on, where the same read on an unbounded chromosome would be
    one = np.array([0, g.genome_len], dtype=np.uint32)
    cut = 0
    for i in range(2, len(meta), 3):
        pos = int(recs["genome_pos"][i])
        inside = int(start[meta[i][0] + 1]) - pos
        assert set(calls[i][inside:]) <= {"."}
        if i % 7 == 2:  # (a sample is enough for the count)
            free, _ = expected_read(g.R, one, seqs[i], pos, 1, meta[i][1], meta[i][2])
            cut += set(free[inside:]) != {"."}
    assert cut >= n // 20, cut


def simulated_reads(g, rng, n_reads, lengths, chroms=None):
    """reads of both conversions and both strands cut from chromosomes long enough, for map_se_rpbat_batch"""
    long_enough = [c for c in (range(g.n_chrom) if chroms is None else chroms) if len(g.seqs[c]) >= max(lengths)]
    out = []
    for _ in range(n_reads):
        c = rng.choice(long_enough)
        ln = rng.choice(lengths)
        at = rng.randrange(0, len(g.seqs[c]) - ln + 1)
        s = g.seqs[c][at:at + ln]
        frm, to = rng.choice([("C", "T"), ("G", "A")])
        s = "".join(to if ch == frm and rng.random() < 0.7 else ch for ch in s)
        out.append(refio.revcomp(s) if rng.random() < 0.5 else s)
    return out


def build_index(g, scratch, tag):
    import walt_amd
    fa, path = os.path.join(scratch, tag + ".fa"), os.path.join(scratch, tag + ".dbindex")
    g.write(fa)
    walt_amd.makedb(fa, path, threads=4)
    db = refio.DbIndex(path)
    R = reference_bases(db)
    assert np.array_equal(db.start_index, g.start_index) and db.names == g.names
    assert R[0].tobytes() == g.R[0].tobytes() and R[1].tobytes() == g.R[1].tobytes()  # N-free: the reference is the FASTA
    db.counter = db.index = None
    idx = walt_amd.Index.open(path, device=0, strands=walt_amd.STRANDS_ALL | walt_amd.WITH_REFERENCE)
    return db, path, idx


def remove_index(path):
    for f in os.listdir(os.path.dirname(path)):
        if f.startswith(os.path.basename(path)):
            os.remove(os.path.join(os.path.dirname(path), f))


# ---------------------------------------------------------------------------
# 1. every look-up path
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module", params=COUNTS)
def contigs(request, scratch):
    import walt_amd
    n_chrom = request.param
    g = contig_genome(n_chrom)
    assert g.n_chrom == n_chrom and min(len(s) for s in g.seqs) == 1 and max(len(s) for s in g.seqs) < 320
    db, path, idx = build_index(g, scratch, "contigs_%d" % n_chrom)
    try:
        seqs, recs, conv, meta = made_up_records(g, 100 + n_chrom)
        # real records beside them: simulated reads through the mapper
        reads = simulated_reads(g, random.Random(n_chrom), 400, [40, 47, 64, 100, 131])
        m_recs, m_conv, _ = idx.map_se_rpbat_batch(*walt_amd.pack_reads(reads))
        assert (m_recs["times"] == 1).sum() > 100
        seqs, recs, conv = seqs + reads, np.concatenate([recs, m_recs]), np.concatenate([conv, m_conv])
        bases, offs = walt_amd.pack_reads(seqs)
        want = expected_batch(db, seqs, recs, conv, R=g.R)
        assert_coverage(g, seqs[:-len(reads)], recs[:-len(reads)], conv[:-len(reads)], meta, want[0][:-len(reads)])
        meth, unmeth = expected_counts(g.R, g.start_index, seqs, recs, conv)
        case = dict(g=g, db=db, idx=idx, seqs=seqs, recs=recs, conv=conv, bases=bases, offs=offs, want=want, meth=meth, unmeth=unmeth)
        case["plain"] = idx.meth_call_batch(bases, offs, recs, conv)
        yield case
    finally:
        idx.close()
        remove_index(path)


def test_calls_on_every_lookup_path(contigs):
    c = contigs
    assert_batch(c["plain"], c["seqs"], c["want"], "%d sequences" % c["g"].n_chrom)
    assert c["want"][2]["reads"] >= 12 * c["g"].n_chrom


@pytest.mark.parametrize("rows", [0, 1])
def test_pileup_on_every_lookup_path(contigs, index_options, rows):
    c = contigs
    g, idx = c["g"], c["idx"]
    index_options(idx, pile_rows=rows)
    pile = idx.pileup()
    try:
        got = pile.add_batch(c["bases"], c["offs"], c["recs"], c["conv"])
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, c["plain"])), "per-read outputs differ from the plain call's"
        sites, off = pile.extract()
        assert_table((sites, off), g.R[0], g.start_index, c["meth"], c["unmeth"], "%d sequences, pile_rows=%d" % (g.n_chrom, rows))
        assert_sums_equal_stats(sites, off, got[2], "%d sequences" % g.n_chrom)
        assert sites.size > 4 * g.n_chrom
        if rows == 0:
            # the device form on a stream writes the same bytes
            import torch
            dev = torch.device("cuda", 0)
            d_sites = torch.full((sites.size + 4, 16), 0x23, dtype=torch.uint8, device=dev)
            d_n = torch.zeros(3, dtype=torch.int64, device=dev)
            stream = torch.cuda.Stream(device=dev)
            torch.cuda.synchronize()
            pile.extract_device(0, g.genome_len, d_sites.data_ptr(), sites.size + 4, d_n.data_ptr(), d_n.data_ptr() + 8,
                                stream=stream.cuda_stream)
            stream.synchronize()
            assert d_n.cpu().numpy().tolist() == [sites.size, 0, 0]
            out = d_sites.cpu().numpy()
            assert out[:sites.size].tobytes() == sites.tobytes() and (out[sites.size:] == 0x23).all()
            if g.n_chrom in RANGE_COUNTS:
                # ranges cut at every chromosome start and at the position before it
                starts = [int(x) for x in g.start_index]
                cuts = sorted(set(starts + [s - 1 for s in starts[1:]]))
                assert cuts[0] == 0 and cuts[-1] == g.genome_len and len(cuts) > g.n_chrom
                parts = [pile.extract(a, b)[0] for a, b in zip(cuts[:-1], cuts[1:])]
                assert np.concatenate(parts).tobytes() == sites.tobytes()
    finally:
        pile.close()


# ---------------------------------------------------------------------------
# 2. a genome larger than one window of the writer, more than 1,024 extraction blocks, and depth
# ---------------------------------------------------------------------------
BIG_LENGTHS = [60] * 1000 + [1500000, 1500000, 1300000] + [60] * 27
STRADDLER = 1002  # the sequence that holds position 2^22


def big_genome():
    rs = np.random.RandomState(4)
    codes = rs.randint(0, 6, size=sum(BIG_LENGTHS)).astype(np.uint8)
    text = np.frombuffer(b"ACGTCG", dtype=np.uint8)[codes].tobytes().decode()
    seqs, at = [], 0
    for L in BIG_LENGTHS:
        seqs.append(text[at:at + L])
        at += L
    return Genome(["b%d" % i for i in range(len(seqs))], seqs)


def big_reads(g):
    """reads of both conversions: spread over every sequence of a megabase, and dense around position 2^22"""
    rng = random.Random(41)
    reads = simulated_reads(g, rng, 1500, [50, 100, 101], chroms=[1000, 1001, 1002])
    lo = int(g.start_index[STRADDLER])
    for at in list(range(WINDOW - 400, WINDOW + 300, 7)):  # on both sides of 2^22 and across it
        s = g.text[at:at + 100]
        frm, to = rng.choice([("C", "T"), ("G", "A")])
        s = "".join(to if ch == frm and rng.random() < 0.7 else ch for ch in s)
        reads.append(refio.revcomp(s) if rng.random() < 0.5 else s)
    assert lo < WINDOW - 400
    reads += simulated_reads(g, rng, 200, [40, 60], chroms=list(range(1000)) + list(range(1003, g.n_chrom)))
    return reads


@pytest.fixture(scope="module")
def big(scratch):
    import walt_amd
    g = big_genome()
    assert g.n_chrom > K_LDS and g.genome_len > WINDOW
    assert int(g.start_index[STRADDLER]) < WINDOW < int(g.start_index[STRADDLER + 1])
    db, path, idx = build_index(g, scratch, "big")
    try:
        reads = big_reads(g)
        fq = os.path.join(scratch, "big.fastq")
        with open(fq, "w") as f:
            for i, s in enumerate(reads):
                f.write("@r%d\n%s\n+\n%s\n" % (i, s, "I" * len(s)))
        loaded = []
        for _, sq, _ in refio.load_fastq_batches(fq, 10 ** 7):
            loaded += sq
        assert loaded == reads
        recs, conv = cli_records_se(idx, loaded, "R")
        uniq = recs["times"] == 1
        assert uniq.sum() > 1500 and {int(c) for c in conv[uniq]} == {ord("T"), ord("A")}
        meth, unmeth = expected_counts(g.R, g.start_index, loaded, recs, conv)
        sites, off = expected_table(g.R[0], g.start_index, meth, unmeth)
        assert off == [0, 0]
        # covered sites in every window, and on both sides of 2^22 inside the sequence that straddles it
        lo, hi = int(g.start_index[STRADDLER]), int(g.start_index[STRADDLER + 1])
        pos = sites["pos"].astype(np.int64)
        assert set((pos // WINDOW).tolist()) == set(range(-(-g.genome_len // WINDOW))) == {0, 1}
        assert ((pos >= lo) & (pos < WINDOW)).sum() > 50 and ((pos >= WINDOW) & (pos < hi)).sum() > 50
        assert pos[pos < WINDOW].max() >= WINDOW - 8 and pos[pos >= WINDOW].min() < WINDOW + 8
        yield dict(g=g, db=db, path=path, idx=idx, fq=fq, seqs=loaded, recs=recs, conv=conv, meth=meth, unmeth=unmeth, sites=sites)
    finally:
        idx.close()
        remove_index(path)


def test_big_extraction_grids_and_device_cap(big, index_options):
    import torch
    import walt_amd
    g, idx = big["g"], big["idx"]
    assert -(-g.genome_len // 4096) > 1024  # the default grid: k_pile_scan sums more than one block per thread
    bases, offs = walt_amd.pack_reads(big["seqs"])
    pile = idx.pileup()
    try:
        _, _, stats = pile.add_batch(bases, offs, big["recs"], big["conv"])
        full, off = pile.extract()
        assert_table((full, off), g.R[0], g.start_index, big["meth"], big["unmeth"], "default grid")
        assert full.tobytes() == big["sites"].tobytes()
        assert_sums_equal_stats(full, off, stats, "big")
        a, b = int(g.start_index[1001]) + 700001, int(g.start_index[STRADDLER]) + 1200001  # mid-chromosome to mid-chromosome, across 2^22
        assert a < WINDOW < b
        part = full[(full["pos"] >= a) & (full["pos"] < b)]
        assert 0 < part.size < full.size
        assert pile.extract(a, b)[0].tobytes() == part.tobytes()
        for blocks in (1, 1025, 4097, 65536):
            index_options(idx, pile_extract_blocks=blocks)
            assert pile.extract()[0].tobytes() == full.tobytes(), blocks
            assert pile.extract(a, b)[0].tobytes() == part.tobytes(), blocks
        index_options(idx, pile_extract_blocks=0)
        # the device form refuses a cap that is one short: the count is set, the guard bytes stay
        dev = torch.device("cuda", 0)
        d_sites = torch.full((full.size, 16), 0x23, dtype=torch.uint8, device=dev)
        d_n = torch.zeros(1, dtype=torch.int64, device=dev)
        stream = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()
        pile.extract_device(0, g.genome_len, d_sites.data_ptr(), full.size - 1, d_n.data_ptr(), None, stream=stream.cuda_stream)
        stream.synchronize()
        assert int(d_n[0]) == full.size and bool((d_sites == 0x23).all())
        pile.extract_device(0, g.genome_len, d_sites.data_ptr(), full.size, d_n.data_ptr(), None, stream=stream.cuda_stream)
        stream.synchronize()
        assert int(d_n[0]) == full.size and d_sites.cpu().numpy().tobytes() == full.tobytes()
    finally:
        pile.close()


def test_big_command_line_two_windows(big, scratch):
    g, db = big["g"], big["db"]
    want_calls = expected_batch(db, big["seqs"], big["recs"], big["conv"], R=g.R)[0]
    text = counts_text(db, big["sites"])
    assert text.count("\n") == big["sites"].size > 1000

    def check(tag, reads_arg, more, copies):
        out = os.path.join(scratch, "big_cli_%s.out" % tag)
        run_walt(["-i", big["path"], "-r", reads_arg, "-o", out, "-sam", "-a", "-u", "-R", "-M", "-MC"] + more)
        assert open(out + ".methcounts").read() == text * copies, tag
        rows = [l for l in open(out) if not l.startswith("@")]
        assert len(rows) == copies * len(big["seqs"])
        n_xm = 0
        for k, line in enumerate(rows):
            i = k % len(big["seqs"])
            _, xm = strip_xm(line)
            mapped = int(big["recs"]["times"][i]) >= 1
            assert (xm is not None) == mapped, (tag, k, line)
            if mapped:
                n_xm += 1
                exp = want_calls[i][::-1] if bytes(big["recs"]["strand"][i]) == b"-" else want_calls[i]
                assert xm == exp, "%s line %d\n got  %s\n want %s" % (tag, k, xm, exp)
        assert n_xm > 1500 * copies

    check("one", big["fq"], [], 1)
    check("g00", big["fq"], ["-g", "0,0"], 1)           # two shares, merged window by window
    check("two", big["fq"] + "," + big["fq"], [], 2)    # one table after another: the counters are cleared between files


def depth_records(g):
    """a read across position 2^22 on '+' and its reverse complement on '-', each under both conversions"""
    import walt_amd
    rng = random.Random(8)
    lo, hi = int(g.start_index[STRADDLER]), int(g.start_index[STRADDLER + 1])
    p, n = WINDOW - 61, 133  # across 2^22, more than one trip, an odd length
    read = list(g.text[p:p + n])
    for i, ch in enumerate(read):  # partly converted both ways: calls under either conversion
        if ch in "CG" and rng.random() < 0.5:
            read[i] = "T" if ch == "C" else "A"
    read = "".join(read)
    rc = refio.revcomp(read)
    recs = np.zeros(4, dtype=walt_amd.best_match_dtype)
    recs["genome_pos"] = [p, lo + hi - (p + n), p, lo + hi - (p + n)]
    recs["times"] = 1
    recs["strand"] = [b"+", b"-", b"+", b"-"]
    conv = np.array([ord(c) for c in "TAAT"], dtype=np.uint8)  # (read, '+', T) and (rc, '-', A) call the same C's; the other two the G's
    assert g.minus[int(recs["genome_pos"][1]):int(recs["genome_pos"][1]) + n] == refio.revcomp(g.text[p:p + n])
    return [read, rc, read, rc], recs, conv, p, n


@pytest.mark.parametrize("rows", [0, 1])
def test_depth_on_one_site_set(big, index_options, rows):
    """four distinct records on one stretch of the genome -- a read on '+' and its reverse complement on '-', each
    under both conversions -- repeated 30,000 times in each of two batches on two streams"""
    import torch
    import walt_amd
    g, idx = big["g"], big["idx"]
    M = 30000
    seqs, recs, conv, p, n = depth_records(g)
    m1, u1 = expected_counts(g.R, g.start_index, seqs, recs, conv)  # the distinct records, once
    want1 = expected_batch(big["db"], seqs, recs, conv, R=g.R)
    covered = (m1 + u1) > 0
    assert int(covered[p:p + n].sum()) == int(covered.sum()) > 30 and covered[WINDOW - 20:WINDOW].any() and covered[WINDOW:WINDOW + 20].any()
    assert int(m1.max()) == 2 and int(u1.max()) == 2  # a site takes the call of the read and of its reverse complement
    # the batch: the four records M times over
    b1, _ = walt_amd.pack_reads(seqs)
    bases = np.tile(b1[:4 * n], M)
    offs = (np.arange(4 * M + 1, dtype=np.uint64) * np.uint64(n))
    big_recs, big_conv = np.tile(recs, M), np.tile(conv, M)
    index_options(idx, pile_rows=rows)
    pile = idx.pileup()
    try:
        dev = torch.device("cuda", 0)
        d_bases = torch.from_numpy(bases).to(dev)
        d_offs = torch.from_numpy(offs.view(np.int64)).to(dev)
        d_recs = torch.from_numpy(big_recs.view(np.uint8).reshape(4 * M, 16)).to(dev)
        d_conv = torch.from_numpy(big_conv).to(dev)
        d_stats = torch.zeros(9, dtype=torch.int64, device=dev)
        streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
        torch.cuda.synchronize()
        # both streams feed the pile-up at the same time; the batch totals are one call at a time per index: the first's
        pile.add_batch_device(d_bases.data_ptr(), d_offs.data_ptr(), 4 * M, d_recs.data_ptr(), 16, d_conv.data_ptr(), 1, "T",
                              d_stats=d_stats.data_ptr(), stream=streams[0].cuda_stream)
        pile.add_batch_device(d_bases.data_ptr(), d_offs.data_ptr(), 4 * M, d_recs.data_ptr(), 16, d_conv.data_ptr(), 1, "T",
                              stream=streams[1].cuda_stream)
        for s in streams:
            s.synchronize()
        sites, off = pile.extract()
        assert_table((sites, off), g.R[0], g.start_index, 2 * M * m1, 2 * M * u1, "depth, pile_rows=%d" % rows)
        assert int(sites["meth"].max()) == 4 * M and int(sites["unmeth"].max()) == 4 * M
        stats = d_stats.cpu().numpy().view(walt_amd.meth_stats_dtype).copy()
        assert int(stats["reads"][0]) == 4 * M
        assert np.array_equal(stats["meth"][0].astype(np.int64), M * want1[2]["meth"])
        assert np.array_equal(stats["unmeth"][0].astype(np.int64), M * want1[2]["unmeth"])
        for f in ("meth", "unmeth"):  # the second batch is the first once more
            stats[f] *= 2
        assert_sums_equal_stats(sites, off, stats, "depth")
    finally:
        pile.close()
