"""The GPU index builder (walt_index_build_device / walt_makedb_device, walt_amd/csrc/build_index.hip) against the
plain restatement of BuildIndex (tests/indexref.py) on the genomes of tests/test_index_builders_cpu.py: a bucket of
exactly 500,000 positions beside one of 499,999 (`erase`), sequences around MINIMALSEEDLEN and unaligned sequence
starts (`edges`), one bucket at every distance from a chromosome end with tie runs and more than 2,048 sequences
(`ends`), and a tie-free genome compared byte for byte (`tiefree`); the builder's strand_mask and dir_bits arguments,
its WALT_EBASE answer, and mapping through the indexes it builds.

Everything is exact, or exact up to the order inside runs of fully equal keys, which come from the restatement.
The restatement of `erase` takes 4.4 s on the CPU (its lexsort is the slowest step here; building that genome on the
device and exporting it takes 3.5 s) and is made once per module."""
import os
import random
import subprocess

import numpy as np
import pytest

import indexref
import refio
from test_harness_cpu import assert_best_equal
from test_index_builders_cpu import Cases

pytestmark = pytest.mark.gpu

GENOMES = ["erase", "edges", "ends", "tiefree"]


@pytest.fixture(scope="module")
def cases(scratch):
    return Cases(scratch)


class Built:
    """Index.build_device of a genome (all strands, default directory), its written files read back, made once"""

    def __init__(self, cases, scratch):
        self.cases, self.scratch, self.made = cases, scratch, {}

    def get(self, name):
        import walt_amd
        if name not in self.made:
            seqs, ref, _, _ = self.cases.get(name)
            d_g = upload(seqs)
            idx = walt_amd.Index.build_device(d_g.data_ptr(), ref.lengths.tolist(), ref.names, device=0)
            path = os.path.join(self.scratch, "ibg_%s.dbindex" % name)
            idx.write(path)
            self.made[name] = (idx, refio.DbIndex(path))
        return self.made[name]

    def close(self):
        for idx, _ in self.made.values():
            idx.close()


@pytest.fixture(scope="module")
def built(cases, scratch):
    b = Built(cases, scratch)
    yield b
    b.close()


def upload(seqs):
    import torch
    return torch.frombuffer(bytearray("".join(s for _, s in seqs).encode()), dtype=torch.uint8).cuda()


@pytest.mark.parametrize("name", GENOMES)
def test_build_device_equals_restatement(cases, built, name):
    _, ref, _, _ = cases.get(name)
    idx, _ = built.get(name)
    assert idx.chrom_names == ref.names and idx.chrom_lengths == ref.lengths.tolist()
    assert idx.genome_len == ref.genome_len
    for s in range(4):
        r = ref.strand[s]
        assert idx.index_size(s) == r.index_size, "strand %d index size" % s
        g, cnt, ix = idx.export_strand(s)
        assert np.array_equal(g, r.genome), "strand %d genome" % s
        assert np.array_equal(cnt, r.counter), "strand %d counter" % s
        assert indexref.same_up_to_ties(ix, r), "strand %d index order" % s
        assert indexref.ascending_in_tie_runs(ix, r), "strand %d order inside tie runs" % s
        if name == "tiefree":
            assert np.array_equal(ix, r.index), "strand %d index" % s


@pytest.mark.parametrize("pattern", [5, 7])
@pytest.mark.parametrize("name", ["edges", "ends"])
def test_build_device_equals_restatement_patterns(cases, name, pattern):
    """Seed patterns 5 and 7 (56 and 80 care characters: pattern 7's low sort keys take two radix passes)"""
    import walt_amd
    seqs, ref, _, _ = cases.get(name, pattern)
    walt_amd.set_pattern(pattern)
    try:
        d_g = upload(seqs)
        idx = walt_amd.Index.build_device(d_g.data_ptr(), ref.lengths.tolist(), ref.names, device=0)
        try:
            for s in range(4):
                r = ref.strand[s]
                assert idx.index_size(s) == r.index_size, "strand %d index size" % s
                g, cnt, ix = idx.export_strand(s)
                assert np.array_equal(g, r.genome), "strand %d genome" % s
                assert np.array_equal(cnt, r.counter), "strand %d counter" % s
                assert indexref.same_up_to_ties(ix, r), "strand %d index order" % s
                assert indexref.ascending_in_tie_runs(ix, r), "strand %d order inside tie runs" % s
        finally:
            idx.close()
    finally:
        walt_amd.set_pattern(3)


@pytest.mark.parametrize("dir_bits", [-1, 24, 28, 32])
@pytest.mark.parametrize("strands", [1, 3, 12, 15])
def test_strand_mask_and_dir_bits(cases, built, scratch, strands, dir_bits):
    """Every resident strand of a partial build, at every directory depth, exports what the all-strand build does; an
    absent strand raises; a C->T-only index writes the head and its two strand files; and reads map through the
    directory of that depth as the oracle maps them."""
    import walt_amd
    seqs, ref, _, _ = cases.get("edges")
    full, full_db = built.get("edges")
    d_g = upload(seqs)
    idx = walt_amd.Index.build_device(d_g.data_ptr(), ref.lengths.tolist(), ref.names, device=0, strands=strands,
                                      dir_bits=dir_bits)
    try:
        if dir_bits >= 0:
            assert idx.dir_bits == dir_bits
        for s in range(4):
            if strands & (1 << s):
                g, cnt, ix = idx.export_strand(s)
                fg, fcnt, fix = full.export_strand(s)
                assert np.array_equal(g, fg) and np.array_equal(cnt, fcnt) and np.array_equal(ix, fix), s
                assert idx.index_size(s) == ref.strand[s].index_size
            else:
                assert idx.index_size(s) == 0
                with pytest.raises(walt_amd.WaltError) as ei:
                    idx.export_strand(s)
                assert ei.value.code == walt_amd.WALT_EINVAL
        if strands == 3:
            d = os.path.join(scratch, "ibg_ctonly_%d" % dir_bits)
            os.makedirs(d)
            idx.write(os.path.join(d, "e.dbindex"))
            assert sorted(os.listdir(d)) == ["e.dbindex", "e.dbindex_CT00", "e.dbindex_CT01"]
            db = refio.DbIndex(os.path.join(d, "e.dbindex"), strands=(0, 1))
            assert db.names == ref.names and np.array_equal(db.lengths, ref.lengths)
            assert db.max_index_size == max(ref.strand[0].index_size, ref.strand[1].index_size)
            for s in (0, 1):
                assert np.array_equal(db.genome[s], ref.strand[s].genome)
                assert np.array_equal(db.counter[s], ref.strand[s].counter)
                assert indexref.same_up_to_ties(db.index[s], ref.strand[s])
        rng = random.Random(31)
        for ag, need in ((False, 3), (True, 12)):
            if strands & need != need:
                continue
            reads = end_reads(rng, seqs, 400, "GA" if ag else "CT")
            want, _ = refio.oracle_se(full_db, reads, ag=ag)
            got, _ = idx.map_se_batch(*walt_amd.pack_reads(reads), ag_wildcard=ag)
            assert_best_equal(got, want, "strands %d dir_bits %d ag %d" % (strands, dir_bits, ag))
    finally:
        idx.close()


@pytest.mark.parametrize("bad,count", [("N", 1), ("c", 1), ("N", 5)])
def test_bad_genome_answers_ebase(bad, count):
    import walt_amd
    rs = np.random.RandomState(32)
    s = list(indexref.random_sequence(rs, 3000))
    for k in range(count):
        s[1000 + 37 * k] = bad
    d_g = upload([("x", "".join(s))])
    with pytest.raises(walt_amd.WaltError) as ei:
        walt_amd.Index.build_device(d_g.data_ptr(), [2000, 1000], ["x", "y"], device=0)
    assert ei.value.code == walt_amd.WALT_EBASE
    assert "genome contains %d non-ACGT bytes" % count in str(ei.value)


# ---------------------------------------------------------------------------
# mapping through the built indexes
# ---------------------------------------------------------------------------
def bisulfite(rng, s, conv):
    """a read of the fragment s: either strand, 90 % conversion, 0 / 1 / 3 % substitutions"""
    a, b = ("C", "T") if conv == "CT" else ("G", "A")
    if rng.random() < 0.5:
        s = refio.revcomp(s)
    s = "".join(b if (c == a and rng.random() < 0.9) else c for c in s)
    rate = rng.choice([0.0, 0.01, 0.03])
    return "".join(rng.choice("ACGT") if rng.random() < rate else c for c in s)


def erase_windows(rng, seqs, runs, n_each, length):
    """(sequence, start) of windows: n_each wholly inside the poly-A run, n_each wholly inside the erased poly-T run,
    n_each straddling an edge of a run, 2 * n_each from the random flanks"""
    out = []
    for which in ("A", "T"):
        c, off, ln = runs[which]
        out += [(c, rng.randrange(off, off + ln - length + 1)) for _ in range(n_each)]
    for _ in range(n_each):
        c, off, ln = runs[rng.choice("AT")]
        out.append((c, rng.choice([off, off + ln]) - rng.randrange(1, length)))
    while len(out) < 5 * n_each:
        c = rng.randrange(len(seqs))
        p = rng.randrange(0, len(seqs[c][1]) - length + 1)
        hit = any(rc == c and p < off + ln and off < p + length for rc, off, ln in runs.values())
        if not hit:
            out.append((c, p))
    return out


def end_reads(rng, seqs, n, conv):
    """reads whose starts lie within 130 bases of their sequence's end"""
    out = []
    long_enough = [s for _, s in seqs if len(s) >= 38]
    while len(out) < n:
        g = rng.choice(long_enough)
        L = rng.randrange(38, min(len(g), 100) + 1)
        p = rng.randrange(max(0, len(g) - 130), len(g) - L + 1)
        out.append(bisulfite(rng, g[p:p + L], conv))
    return out


def assert_pairs_equal(res, want, what):
    for f in ("best_times", "frag_len", "best_i", "best_j", "pair_mm"):
        assert np.array_equal(res[f], want[f]), (what, f)
    assert_best_equal(res["m1"], want["m1"], what + " m1")
    assert_best_equal(res["m2"], want["m2"], what + " m2")


@pytest.fixture(scope="module")
def erase_read_sets(cases):
    seqs, _, _, _ = cases.get("erase")
    runs = indexref.genome_erase()[1]
    rng = random.Random(33)
    sets = {}
    for conv in ("CT", "GA"):
        sets[conv] = [bisulfite(rng, seqs[c][1][p:p + 100], conv) for c, p in erase_windows(rng, seqs, runs, 300, 100)]
    s1, s2 = [], []
    for c, p in erase_windows(rng, seqs, runs, 60, 400):
        frag = seqs[c][1][p:p + rng.randrange(120, 401)]
        if rng.random() < 0.5:
            frag = refio.revcomp(frag)
        frag = "".join("T" if (ch == "C" and rng.random() < 0.9) else ch for ch in frag)
        s1.append(frag[:100])
        s2.append(refio.revcomp(frag)[:100])
    sets["pairs"] = (s1, s2)
    return sets


def open_both(built, cases, name):
    import walt_amd
    dev_idx, dev_db = built.get(name)
    host_path = cases.get(name)[3]
    return [("device-built", dev_idx, dev_db, False),
            ("host-built", walt_amd.Index.open(host_path, device=0), refio.DbIndex(host_path), True)]


@pytest.mark.parametrize("conv", ["CT", "GA"])
def test_erase_single_end_equals_oracle(cases, built, erase_read_sets, conv):
    """1,500 reads of 100 bases: 300 inside the poly-A run (one bucket of 499,999 equal keys; the region exceeds -b),
    300 inside the erased poly-T run (every seed hashes into an empty bucket), 300 across a run's edge, 600 elsewhere."""
    import walt_amd
    reads = erase_read_sets[conv]
    assert len(reads) == 1500
    for what, idx, db, mine in open_both(built, cases, "erase"):
        try:
            want, work = refio.oracle_se(db, reads, ag=conv == "GA")
            got, stats = idx.map_se_batch(*walt_amd.pack_reads(reads), ag_wildcard=conv == "GA")
            assert_best_equal(got, want, "erase %s %s" % (conv, what))
            assert int(stats["too_short"]) == int(work["too_short"])
            # not a vacuous comparison: a third of the reads carry no substitution, and those of them that do not lie
            # wholly inside a run (900 of 1,500 reads, so 300 +- 14) match the genome exactly
            assert int((want["times"] > 0).sum()) > 250
        finally:
            if mine:
                idx.close()


@pytest.mark.parametrize("top_k", [5, 50])
def test_erase_paired_end_equals_oracle(cases, built, erase_read_sets, top_k):
    import walt_amd
    s1, s2 = erase_read_sets["pairs"]
    assert len(s1) == 300
    for what, idx, db, mine in open_both(built, cases, "erase"):
        try:
            want, _, _ = refio.oracle_pe(db, s1, s2, top_k=top_k)
            res, _ = idx.map_pe_batch(*walt_amd.pack_reads(s1), *walt_amd.pack_reads(s2), top_k=top_k)
            assert_pairs_equal(res, want, "erase pairs k=%d %s" % (top_k, what))
            assert int((want["best_times"] > 0).sum()) > 100  # the 120 fragments of the random flanks are exact copies
        finally:
            if mine:
                idx.close()


def test_ends_single_end_equals_oracle(cases, built):
    """1,500 reads per conversion whose starts lie within 130 bases of a chromosome end"""
    import walt_amd
    seqs = cases.get("ends")[0]
    rng = random.Random(34)
    sets = [(False, end_reads(rng, seqs, 1500, "CT")), (True, end_reads(rng, seqs, 1500, "GA"))]
    for what, idx, db, mine in open_both(built, cases, "ends"):
        try:
            for ag, reads in sets:
                want, work = refio.oracle_se(db, reads, ag=ag)
                got, stats = idx.map_se_batch(*walt_amd.pack_reads(reads), ag_wildcard=ag)
                assert_best_equal(got, want, "ends ag=%d %s" % (ag, what))
                assert int(stats["too_short"]) == int(work["too_short"])
                # not a vacuous comparison: a third of the reads (500 +- 18) carry no substitution and match exactly
                assert int((want["times"] > 0).sum()) > 400
        finally:
            if mine:
                idx.close()


# ---------------------------------------------------------------------------
# walt_makedb_device: FASTA -> GPU builder -> files
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["erase", "ends"])
def test_makedb_device_files(cases, scratch, erase_read_sets, name):
    import walt_amd
    seqs, ref, fa, host = cases.get(name)
    out = os.path.join(scratch, "ibg_mk_%s.dbindex" % name)
    rc = walt_amd.lib().walt_makedb_device(fa.encode(), out.encode(), 0)
    assert rc == 0, walt_amd.lib().walt_last_error()
    with open(host, "rb") as f, open(out, "rb") as g:
        assert f.read() == g.read()  # the head file
    a, b = refio.DbIndex(host), refio.DbIndex(out)
    for s in range(4):
        with open(out + refio.STRAND_SUFFIX[s], "rb") as f:
            assert f.read(1) == (b"-" if s & 1 else b"+")
        assert np.array_equal(a.genome[s], b.genome[s]) and np.array_equal(a.counter[s], b.counter[s]), s
        assert a.index[s].size == b.index[s].size
        bucket = np.repeat(np.arange(refio.NUM_BUCKETS, dtype=np.int64), np.diff(a.counter[s].astype(np.int64)))
        for db in (a, b):  # per-bucket multisets
            db.sorted_in_bucket = db.index[s][np.lexsort([db.index[s], bucket])]
        assert np.array_equal(a.sorted_in_bucket, b.sorted_in_bucket), s
        assert indexref.same_up_to_ties(b.index[s], ref.strand[s]), s
        assert indexref.ascending_in_tie_runs(b.index[s], ref.strand[s]), s
    if os.path.exists(refio.REF_WALT):  # the real binary maps from the GPU-written files to the same SAM
        reads = erase_read_sets["CT"][::3] if name == "erase" else end_reads(random.Random(35), seqs, 500, "CT")
        assert len(reads) == 500
        idx = walt_amd.Index.open(out, device=0)
        try:
            got, _ = idx.map_se_batch(*walt_amd.pack_reads(reads))
        finally:
            idx.close()
        fq, sam = os.path.join(scratch, "ibg_mk_%s.fastq" % name), os.path.join(scratch, "ibg_mk_%s.sam" % name)
        with open(fq, "w") as f:
            for i, r in enumerate(reads):
                f.write("@r%d\n%s\n+\n%s\n" % (i, r, "I" * len(r)))
        subprocess.run([refio.REF_WALT, "-i", out, "-r", fq, "-o", sam, "-sam", "-a", "-u"], check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        mine = refio.sam_header(b)
        for i, (rec, r) in enumerate(zip(got, reads)):
            mine += refio.se_sam_line(b, rec, "r%d" % i, r, "I" * len(r), True, True)
        with open(sam) as f:
            assert f.read() == mine
