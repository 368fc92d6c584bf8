"""Per-cytosine methylation pile-up (walt_pileup_*, walt_meth_pileup_batch, bin/walt -MC; the contract is in
include/walt_amd.h, "methylation pile-up").

The expected values come from the restatement below: `expected_read` of tests/test_gpu_meth.py gives the letters of a
record, every letter of every record with times == 1 is walked to its forward position, and the strand and context of a
covered position are classified a second time from the '+' reference alone.  On N-free genomes the restatement itself
asserts that each letter's context equals its site's.  No position is left out: the whole extracted table is compared
with the whole expected table, and both are also compared as dense arrays over every position of the genome.  The
planted-genome test carries expected sites written by hand."""
import os
import random
import subprocess

import numpy as np
import pytest

import refio
from test_gpu_meth import (CONTEXTS, READ_A2, READ_T, _pad_read, _rnd, cli_records_se, clip_point, expected_read, load,
                           planted, reference_bases, run_walt)

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------
def chrom_of(start_index, f):
    c = int(np.searchsorted(start_index, f, side="right")) - 1
    return c, int(start_index[c]), int(start_index[c + 1])


def site_class(R0, start_index, f):
    """-> None where R[f] is A or T, else (strand character, context 0 CpG / 1 CHG / 2 CHH / 3 unknown)."""
    b = chr(R0[f])
    if b not in "CG":
        return None
    _, lo, hi = chrom_of(start_index, f)
    step, key, strand = (1, "G", "+") if b == "C" else (-1, "C", "-")
    q1, q2 = f + step, f + 2 * step
    if not lo <= q1 < hi:
        return strand, 3
    if chr(R0[q1]) == key:
        return strand, 0
    if not lo <= q2 < hi:
        return strand, 3
    return strand, 1 if chr(R0[q2]) == key else 2


def expected_counts(R, start_index, seqs, recs, conv, call_len=None, n_free=True, into=None):
    """(meth, unmeth) int64 arrays over every forward position: the letters of every record with times == 1."""
    glen = len(R[0])
    meth, unmeth = into if into is not None else (np.zeros(glen, dtype=np.int64), np.zeros(glen, dtype=np.int64))
    for i, s in enumerate(seqs):
        if int(recs["times"][i]) != 1:
            continue
        cv = conv if isinstance(conv, str) else chr(int(conv[i]))
        pos, strand = int(recs["genome_pos"][i]), bytes(recs["strand"][i])
        calls, _ = expected_read(R, start_index, s, pos, 1, strand, cv, None if call_len is None else call_len[i])
        if set(calls) <= {"."}:
            continue
        _, lo, hi = chrom_of(start_index, pos)
        for k, ch in enumerate(calls):
            if ch == ".":
                continue
            q = pos + k
            f = lo + hi - 1 - q if strand == b"-" else q
            assert lo <= f < hi
            (meth if ch.isupper() else unmeth)[f] += 1
            if n_free:  # every letter that lands on a site carries the site's context and lies on its strand's base
                cls = site_class(R[0], start_index, f)
                assert cls is not None and cls[1] == "zxhu".index(ch.lower()), (i, k, ch, f, cls)
                assert cls[0] == ("+" if (strand == b"-") == (cv == "A") else "-"), (i, k, ch, strand, cv, cls)
    return meth, unmeth


def expected_table(R0, start_index, meth, unmeth):
    """-> (sites in walt_amd.meth_site_dtype, ascending; [off-reference meth, unmeth])."""
    import walt_amd
    rows, off = [], [0, 0]
    for f in np.nonzero((meth + unmeth) > 0)[0]:
        cls = site_class(R0, start_index, int(f))
        if cls is None:
            off[0] += int(meth[f])
            off[1] += int(unmeth[f])
        else:
            rows.append((int(f), int(meth[f]), int(unmeth[f]), ord(cls[0]), cls[1], 0))
    return np.array(rows, dtype=walt_amd.meth_site_dtype), off


def assert_table(got, R0, start_index, meth, unmeth, what="", lo=0, hi=None):
    """got: (sites, offref) of Pileup.extract over [lo, hi); the expected arrays cover the whole genome."""
    import walt_amd
    hi = len(R0) if hi is None else hi
    sites, off = got
    m, u = meth.copy(), unmeth.copy()
    m[:lo] = 0; u[:lo] = 0; m[hi:] = 0; u[hi:] = 0
    want, woff = expected_table(R0, start_index, m, u)
    assert sites.dtype == walt_amd.meth_site_dtype
    if sites.tobytes() != want.tobytes():
        n = min(len(sites), len(want))
        bad = [k for k in range(n) if sites[k].tobytes() != want[k].tobytes()][:5]
        raise AssertionError("%s: %d sites against %d expected; first differences %s" % (
            what, len(sites), len(want), [(sites[k], want[k]) for k in bad]))
    assert [int(off[0]), int(off[1])] == woff, (what, off, woff)
    # the same as dense arrays: covered and uncovered positions alike
    gm, gu = np.zeros(len(R0), dtype=np.int64), np.zeros(len(R0), dtype=np.int64)
    gm[sites["pos"]] = sites["meth"]
    gu[sites["pos"]] = sites["unmeth"]
    on_ref = np.isin(R0, np.frombuffer(b"CG", dtype=np.uint8))
    assert np.array_equal(gm, np.where(on_ref, m, 0)) and np.array_equal(gu, np.where(on_ref, u, 0)), what
    assert (np.diff(sites["pos"].astype(np.int64)) > 0).all()
    return sites


def context_sums(sites):
    m, u = np.zeros(4, dtype=np.int64), np.zeros(4, dtype=np.int64)
    for k in range(4):
        sel = sites["context"] == k
        m[k], u[k] = int(sites["meth"][sel].sum()), int(sites["unmeth"][sel].sum())
    return m, u


def assert_sums_equal_stats(sites, off, stats, what=""):
    m, u = context_sums(sites)
    assert int(off[0]) == 0 and int(off[1]) == 0, (what, off)
    assert np.array_equal(m, stats["meth"][0].astype(np.int64)) and np.array_equal(u, stats["unmeth"][0].astype(np.int64)), (what, m, u, stats)


def counts_text(db, sites):
    out = []
    for s in sites:
        c, lo, _ = chrom_of(db.start_index, int(s["pos"]))
        out.append("%s\t%d\t%s\t%s\t%d\t%d\n" % (db.names[c], int(s["pos"]) - lo, chr(int(s["strand"])), CONTEXTS[int(s["context"])],
                                                   int(s["meth"]), int(s["unmeth"])))
    return "".join(out)


# ---------------------------------------------------------------------------
# 1. the golden libraries
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g1(scratch):
    import walt_amd
    path = os.path.join(scratch, "pile_g1.dbindex")
    walt_amd.makedb(os.path.join(refio.GOLDEN, "g1.fa"), path, threads=4)
    return refio.DbIndex(path), path


@pytest.fixture(scope="module")
def g1_all(g1):
    import walt_amd
    idx = walt_amd.Index.open(g1[1], device=0, strands=walt_amd.STRANDS_ALL | walt_amd.WITH_REFERENCE)
    yield idx
    idx.close()


def check_library(idx, db, batches, what):
    """batches: (seqs, bases, offs, recs, conv) fed one after the other into ONE pile-up.  The table equals the
    restatement, its per-context sums the totals of the same calls, the per-read outputs are meth_call_batch's, a
    second round doubles every count and clear() empties the table."""
    R = reference_bases(db)
    pile = idx.pileup()
    try:
        assert pile.extract()[0].size == 0
        meth = unmeth = None
        stats = None
        for seqs, bases, offs, recs, conv in batches:
            got = pile.add_batch(bases, offs, recs, conv, stats=stats)
            stats = got[2]
            plain = idx.meth_call_batch(bases, offs, recs, conv)
            assert got[0].tobytes() == plain[0].tobytes() and got[1].tobytes() == plain[1].tobytes(), what
            meth, unmeth = expected_counts(R, db.start_index, seqs, recs, conv, into=None if meth is None else (meth, unmeth))
        ref_stats = None
        for seqs, bases, offs, recs, conv in batches:
            ref_stats = idx.meth_call_batch(bases, offs, recs, conv, want_calls=False, want_counts=False, stats=ref_stats)[2]
        assert stats.tobytes() == ref_stats.tobytes(), what
        sites = assert_table(pile.extract(), R[0], db.start_index, meth, unmeth, what)
        assert sites.size > 100
        assert_sums_equal_stats(sites, pile.extract()[1], stats, what)
        for seqs, bases, offs, recs, conv in batches:  # only the pile-up is fed
            c, k, s = pile.add_batch(bases, offs, recs, conv, want_calls=False, want_counts=False, want_stats=False)
            assert c is None and k is None and s is None
        assert_table(pile.extract(), R[0], db.start_index, 2 * meth, 2 * unmeth, what + " twice")
        pile.clear()
        sites, off = pile.extract()
        assert sites.size == 0 and int(off[0]) == 0 and int(off[1]) == 0
        return meth, unmeth
    finally:
        pile.close()


def test_golden_se_ct(g1):
    import walt_amd
    db, path = g1
    idx = walt_amd.Index.open(path, device=0, strands=walt_amd.STRANDS_CT | walt_amd.WITH_REFERENCE)
    try:
        _, seqs, _ = load("se_ct.fastq")
        bases, offs = walt_amd.pack_reads(seqs)
        recs, _ = idx.map_se_batch(bases, offs)
        assert int((recs["times"] == 1).sum()) == 987 and int((recs["times"] >= 2).sum()) > 0
        check_library(idx, db, [(seqs, bases, offs, recs, "T")], "se_ct")
    finally:
        idx.close()


def test_golden_se_ga(g1):
    import walt_amd
    db, path = g1
    idx = walt_amd.Index.open(path, device=0, strands=walt_amd.STRANDS_GA | walt_amd.WITH_REFERENCE)
    try:
        _, seqs, _ = load("se_ga.fastq")
        bases, offs = walt_amd.pack_reads(seqs)
        recs, _ = idx.map_se_batch(bases, offs, ag_wildcard=True)
        check_library(idx, db, [(seqs, bases, offs, recs, "A")], "se_ga")
    finally:
        idx.close()


def test_golden_mixed_library_with_conv_array(g1, g1_all):
    import walt_amd
    from test_gpu_rpbat import mixed_library
    db, _ = g1
    _, seqs, _ = mixed_library()
    bases, offs = walt_amd.pack_reads(seqs)
    recs, conv, _ = g1_all.map_se_rpbat_batch(bases, offs)
    assert (conv == ord("T")).sum() > 100 and (conv == ord("A")).sum() > 100
    meth, unmeth = check_library(g1_all, db, [(seqs, bases, offs, recs, conv)], "mixed -R")
    # all four combinations of strand and conversion piled up, and both kinds of site exist
    uniq = recs["times"] == 1
    assert {(bytes(s), int(c)) for s, c in zip(recs["strand"][uniq], conv[uniq])} == {(b"+", 84), (b"-", 84), (b"+", 65), (b"-", 65)}


@pytest.mark.parametrize("files", [("pe_1.fastq", "pe_2.fastq"), ("pe150_1.fastq", "pe150_2.fastq")])
def test_golden_pairs_both_mates_into_one_pileup(g1, g1_all, files):
    import walt_amd
    db, _ = g1
    _, s1, _ = load(files[0])
    _, s2, _ = load(files[1])
    b1, o1 = walt_amd.pack_reads(s1)
    b2, o2 = walt_amd.pack_reads(s2)
    out, _ = g1_all.map_pe_batch(b1, o1, b2, o2)
    assert out["m1"].strides[0] == 64
    check_library(g1_all, db, [(s1, b1, o1, out["m1"], "T"), (s2, b2, o2, out["m2"], "A")], files[0])


@pytest.mark.parametrize("pattern", [5, 7])
def test_golden_seed_patterns_5_and_7(scratch, pattern):
    import walt_amd
    old = walt_amd.PATTERN
    walt_amd.set_pattern(pattern)
    refio.set_pattern(pattern)
    try:
        path = os.path.join(scratch, "pile_g1_sp%d.dbindex" % pattern)
        walt_amd.makedb(os.path.join(refio.GOLDEN, "g1.fa"), path, threads=4)
        db = refio.DbIndex(path)
        idx = walt_amd.Index.open(path, device=0, strands=walt_amd.STRANDS_ALL | walt_amd.WITH_REFERENCE)
        try:
            batches = []
            for name, ag in (("sp_se_ct.fastq", False), ("sp_se_ga.fastq", True)):
                _, seqs, _ = load(name)
                bases, offs = walt_amd.pack_reads(seqs)
                recs, _ = idx.map_se_batch(bases, offs, ag_wildcard=ag)
                batches.append((seqs, bases, offs, recs, "A" if ag else "T"))
            check_library(idx, db, batches, "pattern %d" % pattern)
        finally:
            idx.close()
    finally:
        walt_amd.set_pattern(old)
        refio.set_pattern(3)


# ---------------------------------------------------------------------------
# 2. the planted genome: expected sites written by hand (the cores of tests/test_gpu_meth.py)
# ---------------------------------------------------------------------------
CpG, CHG, CHH, UNKNOWN = 0, 1, 2, 3


def core_sites(sites, at):
    sel = (sites["pos"] >= at) & (sites["pos"] < at + 60)
    return [(int(s["pos"]) - at, chr(int(s["strand"])), int(s["context"]), int(s["meth"]), int(s["unmeth"])) for s in sites[sel]]


def test_planted_genome_hand_written_sites(scratch):
    import walt_amd
    fa, p1, short, chr_e = planted(scratch)
    path = os.path.join(scratch, "pile_planted.dbindex")
    walt_amd.makedb(fa, path, threads=4)
    db = refio.DbIndex(path)
    idx = walt_amd.Index.open(path, device=0, strands=walt_amd.STRANDS_ALL | walt_amd.WITH_REFERENCE)
    pile = idx.pileup()
    try:
        at_t, at_a2 = 400, 400 + 60 + 300 + 60 + 300
        # READ_T on '+': C kept at 5, 19, 31 (methylated), T at 12, 25, 38; contexts CpG CHG CHH CpG CHG CHH
        read = _pad_read(READ_T, p1, at_t, 20, 20, "T")
        bases, offs = walt_amd.pack_reads([read])
        recs, _ = idx.map_se_batch(bases, offs)
        assert int(recs["times"][0]) == 1 and int(recs["genome_pos"][0]) == at_t - 20 and recs["strand"][0] == b"+"
        pile.add_batch(bases, offs, recs, "T")
        want_t = [(5, "+", CpG, 1, 0), (12, "+", CHG, 0, 1), (19, "+", CHH, 1, 0), (25, "+", CpG, 0, 1), (31, "+", CHG, 1, 0),
                  (38, "+", CHH, 0, 1)]
        assert core_sites(pile.extract()[0], at_t) == want_t
        # its reverse complement maps on '-' under conversion 'A' and piles onto the same six sites
        rc_read = refio.revcomp(read)
        bases, offs = walt_amd.pack_reads([rc_read])
        recs, _ = idx.map_se_batch(bases, offs, ag_wildcard=True)
        assert int(recs["times"][0]) == 1 and recs["strand"][0] == b"-"
        pile.add_batch(bases, offs, recs, "A")
        assert core_sites(pile.extract()[0], at_t) == [(p, s, c, 2 * m, 2 * u) for p, s, c, m, u in want_t]
        # READ_A2 under 'A': G kept at 4, 17, 28, 42, A at 11, 22, 35: sites of the '-' strand
        pile.clear()
        read = _pad_read(READ_A2, p1, at_a2, 20, 20, "A")
        bases, offs = walt_amd.pack_reads([read])
        recs, _ = idx.map_se_batch(bases, offs, ag_wildcard=True)
        assert int(recs["times"][0]) == 1 and int(recs["genome_pos"][0]) == at_a2 - 20 and recs["strand"][0] == b"+"
        pile.add_batch(bases, offs, recs, "A")
        assert core_sites(pile.extract()[0], at_a2) == [
            (4, "-", CpG, 1, 0), (11, "-", CHG, 0, 1), (17, "-", CHG, 1, 0), (22, "-", CpG, 0, 1), (28, "-", CHG, 1, 0),
            (35, "-", CHG, 0, 1), (42, "-", CpG, 1, 0)]
        # chrE ends TACATCC: a made-up record on the last base; the last two C have no context inside the chromosome
        pile.clear()
        e0, e_len = int(db.start_index[2]), len(chr_e)
        tail = chr_e[-60:]
        bases, offs = walt_amd.pack_reads([tail[:-7].replace("C", "T") + "TACATCC"])
        recs = np.zeros(1, dtype=walt_amd.best_match_dtype)
        recs["genome_pos"], recs["times"], recs["strand"] = e0 + e_len - 60, 1, b"+"
        pile.add_batch(bases, offs, recs, "T")
        sites, _ = pile.extract()
        end = e0 + e_len
        assert [(int(s["pos"]) - end, chr(int(s["strand"])), int(s["context"]), int(s["meth"]), int(s["unmeth"]))
                for s in sites[sites["pos"] >= end - 7]] == [(-5, "+", CHH, 1, 0), (-2, "+", UNKNOWN, 1, 0), (-1, "+", UNKNOWN, 1, 0)]
        # times == 2 and a position beyond the genome add nothing
        before = pile.extract()[0].tobytes()
        for pos, times in ((e0 + e_len - 60, 2), (db.genome_len, 1), (0xFFFFFFF0, 1)):
            recs["genome_pos"], recs["times"] = pos, times
            pile.add_batch(bases, offs, recs, "T")
        assert pile.extract()[0].tobytes() == before
    finally:
        pile.close()
        idx.close()


# ---------------------------------------------------------------------------
# 3. ranges
# ---------------------------------------------------------------------------
def test_ranges_caps_and_grid_sizes(g1, g1_all, index_options):
    import ctypes
    import walt_amd
    db, _ = g1
    R = reference_bases(db)
    _, seqs, _ = load("se_ct.fastq")
    bases, offs = walt_amd.pack_reads(seqs)
    recs, _ = g1_all.map_se_batch(bases, offs)
    meth, unmeth = expected_counts(R, db.start_index, seqs, recs, "T")
    pile = g1_all.pileup()
    try:
        pile.add_batch(bases, offs, recs, "T", want_calls=False, want_counts=False, want_stats=False)
        full, _ = pile.extract()
        glen = db.genome_len
        rng = random.Random(3)
        starts = [int(x) for x in db.start_index]
        for cuts in ([0, glen], [0, 1, 2, glen - 1, glen], [0] + sorted(rng.sample(range(1, glen), 9)) + [glen],
                     sorted(set(starts + [s + 1 for s in starts[:-1]] + [max(s - 1, 0) for s in starts]))):
            parts = [pile.extract(a, b)[0] for a, b in zip(cuts[:-1], cuts[1:])]
            assert np.concatenate(parts).tobytes() == full.tobytes(), cuts
        # a range that cuts a chromosome in the middle of covered ground, checked against the restatement
        mid = int(full["pos"][full.size // 2])
        assert_table(pile.extract(mid - 1, mid + 2), R[0], db.start_index, meth, unmeth, "cut", mid - 1, mid + 2)
        assert pile.extract(mid, mid)[0].size == 0
        # a cap that is too small: WALT_EINVAL, n_sites set, nothing written
        L = walt_amd.lib()
        n = ctypes.c_uint64(0)
        buf = np.full(full.size, 0x23, dtype=np.uint8).repeat(16).view(walt_amd.meth_site_dtype)
        rc = L.walt_pileup_extract(pile.handle, 0, glen, buf.ctypes.data, full.size - 1, ctypes.byref(n), None)
        assert rc == walt_amd.WALT_EINVAL and n.value == full.size
        msg = L.walt_last_error().decode()
        assert str(full.size) in msg and str(full.size - 1) in msg, msg
        assert (buf.view(np.uint8) == 0x23).all()
        rc = L.walt_pileup_extract(pile.handle, 0, glen, buf.ctypes.data, full.size, ctypes.byref(n), None)
        assert rc == 0 and buf.tobytes() == full.tobytes()
        # bad ranges
        assert L.walt_pileup_extract(pile.handle, 5, 4, None, 0, ctypes.byref(n), None) == walt_amd.WALT_EINVAL
        assert L.walt_pileup_extract(pile.handle, 0, glen + 1, None, 0, ctypes.byref(n), None) == walt_amd.WALT_EINVAL
        assert b"range" in L.walt_last_error()
        # the table does not depend on the launch shape
        for blocks in (1, 7, 1000):
            index_options(g1_all, pile_extract_blocks=blocks)
            assert pile.extract()[0].tobytes() == full.tobytes(), blocks
            assert pile.extract(mid - 100, mid + 1000)[0].tobytes() == full[(full["pos"] >= mid - 100) & (full["pos"] < mid + 1000)].tobytes()
    finally:
        pile.close()


def test_both_add_shapes_give_the_same_table(g1, g1_all, index_options):
    """pile_rows (neighbouring lanes on neighbouring positions) and the default (a lane per slice), '-' strand included"""
    import walt_amd
    from test_gpu_rpbat import mixed_library
    db, _ = g1
    R = reference_bases(db)
    _, seqs, _ = mixed_library()
    bases, offs = walt_amd.pack_reads(seqs)
    recs, conv, _ = g1_all.map_se_rpbat_batch(bases, offs)
    rng = random.Random(11)
    call_len = [rng.choice([len(s), len(s), len(s) // 2, 0, len(s) + 3]) for s in seqs]
    meth, unmeth = expected_counts(R, db.start_index, seqs, recs, conv, call_len)
    plain = g1_all.meth_call_batch(bases, offs, recs, conv, call_len=call_len)
    for rows in (0, 1):
        index_options(g1_all, pile_rows=rows)
        pile = g1_all.pileup()
        try:
            got = pile.add_batch(bases, offs, recs, conv, call_len=call_len)
            assert all(g.tobytes() == p.tobytes() for g, p in zip(got, plain)), rows
            assert_table(pile.extract(), R[0], db.start_index, meth, unmeth, "pile_rows=%d" % rows)
            pile.add_batch(bases, offs, recs, conv, call_len=call_len, want_calls=False, want_counts=False, want_stats=False)
            assert_table(pile.extract(), R[0], db.start_index, 2 * meth, 2 * unmeth, "pile_rows=%d, pile-up alone" % rows)
        finally:
            pile.close()


# ---------------------------------------------------------------------------
# 4. a FASTA with a run of N: independent fills in the strand files
# ---------------------------------------------------------------------------
def test_fasta_with_a_run_of_n(scratch):
    import walt_amd
    rng = random.Random(9)
    a, b = _rnd(rng, 3000), _rnd(rng, 3000)
    fa = os.path.join(scratch, "pile_n.fa")
    with open(fa, "w") as f:
        f.write(">n1\n%s%s%s\n>n2\n%s\n" % (a, "N" * 40, b, _rnd(rng, 1500)))
    path = os.path.join(scratch, "pile_n.dbindex")
    walt_amd.makedb(fa, path, threads=4)
    db = refio.DbIndex(path)
    R = reference_bases(db)
    idx = walt_amd.Index.open(path, device=0, strands=walt_amd.STRANDS_ALL | walt_amd.WITH_REFERENCE)
    pile = idx.pileup()
    try:
        seqs, convs = [], []
        for k in (0, 2, 4, 6):  # reads that run into the N run from both sides, of both strands
            for s in (a[-(100 - k):].replace("C", "T") + _rnd(rng, k, "AT"), _rnd(rng, k, "AT") + b[:100 - k].replace("C", "T")):
                seqs += [s, refio.revcomp(s)]
        bases, offs = walt_amd.pack_reads(seqs)
        recs, conv, _ = idx.map_se_rpbat_batch(bases, offs)
        assert (recs["times"] == 1).sum() >= 8 and {b"+", b"-"} <= set(recs["strand"][recs["times"] == 1].tolist())
        # made-up records that lie inside the N run on both strands: calls on the fills as the files hold them
        lo, hi = int(db.start_index[0]), int(db.start_index[1])
        extra = []
        for strand, cv in ((b"+", "T"), (b"+", "A"), (b"-", "T"), (b"-", "A")):
            p = 3000 - 30 if strand == b"+" else lo + hi - (3000 + 40 + 30)
            G = R[1 if strand == b"-" else 0]
            extra.append(("".join(chr(c) for c in G[p:p + 100]), p, strand, cv))
        seqs += [e[0] for e in extra]
        bases, offs = walt_amd.pack_reads(seqs)
        recs = np.concatenate([recs, np.zeros(len(extra), dtype=walt_amd.best_match_dtype)])
        conv = np.concatenate([conv, np.zeros(len(extra), dtype=np.uint8)])
        for j, e in enumerate(extra):
            k = len(seqs) - len(extra) + j
            recs["genome_pos"][k], recs["times"][k], recs["strand"][k], conv[k] = e[1], 1, e[2], ord(e[3])
        _, _, stats = pile.add_batch(bases, offs, recs, conv)
        meth, unmeth = expected_counts(R, db.start_index, seqs, recs, conv, n_free=False)
        sites, off = pile.extract()
        assert_table((sites, off), R[0], db.start_index, meth, unmeth, "N run")
        # reported plus off-reference calls equal the totals
        assert int(sites["meth"].sum()) + int(off[0]) == int(stats["meth"][0].sum())
        assert int(sites["unmeth"].sum()) + int(off[1]) == int(stats["unmeth"][0].sum())
    finally:
        pile.close()
        idx.close()


# ---------------------------------------------------------------------------
# 5. device form
# ---------------------------------------------------------------------------
def test_device_form_streams_bytes_and_refusals(g1, g1_all):
    import torch
    import walt_amd
    db, path = g1
    _, seqs, _ = load("se_ct.fastq")
    bases, offs = walt_amd.pack_reads(seqs)
    recs, _ = g1_all.map_se_batch(bases, offs)
    n = len(seqs)
    host_pile = g1_all.pileup()
    pile = g1_all.pileup()
    try:
        assert pile.device_bytes == 8 * db.genome_len + (1 << 20)
        host = host_pile.add_batch(bases, offs, recs, "T")
        want, _ = host_pile.extract()
        dev = torch.device("cuda", 0)
        d_bases = torch.from_numpy(bases).to(dev)
        d_offs = torch.from_numpy(offs.view(np.int64)).to(dev)
        d_recs = torch.from_numpy(recs.view(np.uint8).reshape(n, 16)).to(dev)
        d_calls = torch.zeros(bases.size + 32, dtype=torch.uint8, device=dev)
        d_counts = torch.zeros((n, 16), dtype=torch.uint8, device=dev)
        d_stats = torch.zeros(9, dtype=torch.int64, device=dev)
        s1, s2 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()
        pile.add_batch_device(d_bases.data_ptr(), d_offs.data_ptr(), n, d_recs.data_ptr(), 16, None, 1, "T", None,
                              d_calls.data_ptr(), d_counts.data_ptr(), d_stats.data_ptr(), stream=s1.cuda_stream)
        # the extraction on the same stream comes after the adds
        d_sites = torch.zeros((want.size + 8, 16), dtype=torch.uint8, device=dev)
        d_n = torch.zeros(3, dtype=torch.int64, device=dev)
        pile.extract_device(0, db.genome_len, d_sites.data_ptr(), want.size + 8, d_n.data_ptr(), d_n.data_ptr() + 8,
                            stream=s1.cuda_stream)
        s1.synchronize()
        assert d_n.cpu().numpy().tolist() == [want.size, 0, 0]
        assert d_sites.cpu().numpy()[:want.size].tobytes() == want.tobytes()
        assert d_calls.cpu().numpy()[:bases.size].tobytes() == host[0].tobytes()
        assert d_counts.cpu().numpy().tobytes() == host[1].tobytes() and d_stats.cpu().numpy().tobytes() == host[2].tobytes()
        # a cap that is too small: the count comes back, nothing is written
        d_sites.fill_(0x23)
        pile.extract_device(0, db.genome_len, d_sites.data_ptr(), want.size - 1, d_n.data_ptr(), None, stream=s1.cuda_stream)
        s1.synchronize()
        assert int(d_n[0]) == want.size and bool((d_sites == 0x23).all())
        # two streams feed one pile-up at the same time: the halves of the batch, pile-up alone
        pile.clear()
        half = n // 2
        d_offs2 = torch.from_numpy((offs[half:] - offs[half]).view(np.int64)).to(dev)
        torch.cuda.synchronize()
        for _ in range(3):
            pile.add_batch_device(d_bases.data_ptr(), d_offs.data_ptr(), half, d_recs.data_ptr(), 16, None, 1, "T",
                                  stream=s1.cuda_stream)
            pile.add_batch_device(d_bases.data_ptr() + int(offs[half]), d_offs2.data_ptr(), n - half,
                                  d_recs.data_ptr() + 16 * half, 16, None, 1, "T", stream=s2.cuda_stream)
        s1.synchronize()
        s2.synchronize()
        got, _ = pile.extract()
        tripled = want.copy()
        tripled["meth"] *= 3
        tripled["unmeth"] *= 3
        assert got.tobytes() == tripled.tobytes()
        # refusals: a pile-up of another index, an index without reference, null handles
        L = walt_amd.lib()
        other = walt_amd.Index.open(path, device=0, strands=walt_amd.STRANDS_CT | walt_amd.WITH_REFERENCE)
        bare = walt_amd.Index.open(path, device=0, strands=walt_amd.STRANDS_CT)
        try:
            rc = L.walt_meth_pileup_batch(other.handle, pile.handle, bases.ctypes.data, offs.ctypes.data, n, recs.ctypes.data, 16,
                                          None, 0, ord("T"), None, None, None, None)
            assert rc == walt_amd.WALT_EINVAL and b"another index" in L.walt_last_error()
            with pytest.raises(walt_amd.WaltError) as ei:
                bare.pileup()
            assert ei.value.code == walt_amd.WALT_EINVAL and "reference" in str(ei.value)
            rc = L.walt_meth_pileup_batch(g1_all.handle, pile.handle, bases.ctypes.data, offs.ctypes.data, n, recs.ctypes.data, 8,
                                          None, 0, ord("T"), None, None, None, None)
            assert rc == walt_amd.WALT_EINVAL and b"stride" in L.walt_last_error()
        finally:
            other.close()
            bare.close()
    finally:
        pile.close()
        host_pile.close()


# ---------------------------------------------------------------------------
# 6. command line
# ---------------------------------------------------------------------------
def side_files(out):
    d, base = os.path.dirname(out), os.path.basename(out)
    return sorted(f[len(base):] for f in os.listdir(d) if f.startswith(base) and not f.endswith(".methcounts"))


def run_variants(scratch, tag, path, reads_args, extra, want_text):
    """-MC with and without -M and -sam: <out>.methcounts is the expected text, every other file is the run's without -MC"""
    for sam in ([], ["-sam"]):
        for m in ([], ["-M"]):
            name = "pile_cli_%s%s%s" % (tag, "_sam" if sam else "", "_M" if m else "")
            base, with_mc = os.path.join(scratch, name + ".base"), os.path.join(scratch, name + ".mc")
            common = ["-i", path] + reads_args + ["-a", "-u"] + extra + sam + m
            run_walt(common + ["-o", base])
            run_walt(common + ["-o", with_mc, "-MC"])
            assert not os.path.exists(base + ".methcounts")
            assert open(with_mc + ".methcounts").read() == want_text, name
            files = side_files(base)
            assert files == side_files(with_mc) and "" in files and ".mapstats" in files and (".methstats" in files) == bool(m)
            for sfx in files:
                assert open(base + sfx, "rb").read() == open(with_mc + sfx, "rb").read(), (name, sfx)


@pytest.mark.parametrize("case", ["se_ct", "se_ga_A", "mixed_R", "se_clip_C"])
def test_cli_single_end(g1, g1_all, scratch, case):
    from test_gpu_rpbat import mixed_library
    db, path = g1
    R = reference_bases(db)
    adaptor = ""
    if case == "se_ct":
        fq, extra, mode = os.path.join(refio.GOLDEN, "se_ct.fastq"), [], "T"
    elif case == "se_ga_A":
        fq, extra, mode = os.path.join(refio.GOLDEN, "se_ga.fastq"), ["-A"], "A"
    elif case == "se_clip_C":
        args = refio.golden_meta()["cases"]["se_clip_sam_au"]["args"]
        adaptor = args[args.index("-C") + 1]
        fq, extra, mode = os.path.join(refio.GOLDEN, "se_clip.fastq"), ["-C", adaptor], "T"
    else:
        names, seqs, scores = mixed_library()
        fq = os.path.join(scratch, "pile_mixed.fastq")
        with open(fq, "w") as f:
            for nm, s, q in zip(names, seqs, scores):
                f.write("@%s\n%s\n+\n%s\n" % (nm, s, q))
        extra, mode = ["-R"], "R"
    loaded = []
    for nm, sq, sc in refio.load_fastq_batches(fq, 10 ** 7, adaptor):
        loaded += sq
    call_len = None
    if adaptor:
        raw_reads = [l.rstrip(b"\n") for l in open(fq, "rb").readlines()[1::4]]
        call_len = [clip_point(adaptor.encode(), bytearray(r)) for r in raw_reads]
        assert sum(c < len(r) for c, r in zip(call_len, raw_reads)) > 10
    recs, conv = cli_records_se(g1_all, loaded, mode)
    meth, unmeth = expected_counts(R, db.start_index, loaded, recs, conv, call_len)
    sites, off = expected_table(R[0], db.start_index, meth, unmeth)
    assert sites.size > 100 and off == [0, 0]
    text = counts_text(db, sites)
    run_variants(scratch, case, path, ["-r", fq], extra, text)
    if case == "se_ct":
        # two read files that share one output name: one table after the other; -v reports the off-reference calls
        out = os.path.join(scratch, "pile_cli_two.out")
        log = run_walt(["-i", path, "-r", fq + "," + fq, "-o", out, "-MC", "-v"])
        assert open(out + ".methcounts").read() == text + text
        assert "off-reference" in log
        # -g 0,0: two shares, two pile-ups, merged on the host
        out = os.path.join(scratch, "pile_cli_g00.out")
        run_walt(["-i", path, "-r", fq, "-o", out, "-MC", "-g", "0,0"])
        assert open(out + ".methcounts").read() == text
        # all three spellings
        for flag in ("-methcounts", "--meth-counts"):
            out = os.path.join(scratch, "pile_cli_spell.out")
            run_walt(["-i", path, "-r", fq, "-o", out, flag])
            assert open(out + ".methcounts").read() == text


@pytest.mark.parametrize("mode", ["pe", "P", "RP"])
def test_cli_paired_end(g1, g1_all, scratch, mode):
    import walt_amd
    db, path = g1
    R = reference_bases(db)
    f1, f2 = os.path.join(refio.GOLDEN, "pe_1.fastq"), os.path.join(refio.GOLDEN, "pe_2.fastq")
    _, s1, _ = load("pe_1.fastq")
    _, s2, _ = load("pe_2.fastq")
    b1, o1 = walt_amd.pack_reads(s1)
    b2, o2 = walt_amd.pack_reads(s2)
    if mode == "pe":
        res, _ = g1_all.map_pe_batch(b1, o1, b2, o2)
        parts = [(s1, res["m1"], "T"), (s2, res["m2"], "A")]
    elif mode == "P":  # a PBAT library: the A-rich mates in the -1 file.  -P maps the -2 file C->T and the -1 file G->A
        f1, f2 = f2, f1
        res, _ = g1_all.map_pe_batch(b1, o1, b2, o2)
        parts = [(s1, res["m1"], "T"), (s2, res["m2"], "A")]
    else:
        res, conv, _ = g1_all.map_pe_rpbat_batch(b1, o1, b2, o2)
        parts = [(s1, res["m1"], conv[:, 0]), (s2, res["m2"], conv[:, 1])]
    acc = None
    for seqs, recs, cv in parts:  # both mates into the same table
        acc = expected_counts(R, db.start_index, seqs, recs, cv, into=acc)
    sites, off = expected_table(R[0], db.start_index, *acc)
    assert sites.size > 1000 and off == [0, 0]
    run_variants(scratch, "pe_" + mode, path, ["-1", f1, "-2", f2], {"pe": [], "P": ["-P"], "RP": ["-RP"]}[mode], counts_text(db, sites))


def test_cli_two_devices(g1, scratch):
    import walt_amd
    if walt_amd.device_count() < 2:
        pytest.skip("one device")
    _, path = g1
    fq = os.path.join(refio.GOLDEN, "se_ct.fastq")
    a, b = os.path.join(scratch, "pile_cli_g0.out"), os.path.join(scratch, "pile_cli_g01.out")
    run_walt(["-i", path, "-r", fq, "-o", a, "-MC", "-g", "0"])
    run_walt(["-i", path, "-r", fq, "-o", b, "-MC", "-g", "0,1"])
    assert open(a + ".methcounts", "rb").read() == open(b + ".methcounts", "rb").read()
