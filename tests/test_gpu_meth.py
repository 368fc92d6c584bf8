"""Per-read methylation calls (walt_meth_call_batch, bin/walt -M; the contract is in include/walt_amd.h).

The expected values come from `expected_read` below, a restatement of the header's table in plain Python over the
strand genomes of the .dbindex files (refio.DbIndex), applied to the records the GPU mapping call returned (those
records are pinned against the oracle by the other test files).  No read is left out of any comparison: calls, counts
and totals are compared for every read of every batch, mapped or not.  The planted-genome test carries expected
strings written by hand, so the restatement and the kernel cannot share a mistake unnoticed."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import refio

pytestmark = pytest.mark.gpu

WALT_BIN = os.path.join(refio.ROOT, "walt_amd", "bin", "walt")
CONTEXTS = ("CpG", "CHG", "CHH", "unknown")


# ---------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------
def reference_bases(db):
    """[R, R']: a position is C exactly where the G->A genome says C, else what the C->T genome says."""
    return [np.where(db.genome[2 + o] == ord("C"), np.uint8(ord("C")), db.genome[o]) for o in (0, 1)]


def expected_read(R, start_index, seq, pos, times, strand, conv, call_len=None):
    """-> (calls str, [meth CpG, CHG, CHH, unknown, unmeth CpG, CHG, CHH, unknown])."""
    n = len(seq)
    counts = [0] * 8
    pos, times = int(pos), int(times)
    if times == 0 or pos >= len(R[0]) or conv not in ("T", "A") or n > 1024:
        return "." * n, counts
    G = R[1 if strand in (b"-", "-") else 0]
    c = int(np.searchsorted(start_index, pos, side="right")) - 1
    lo, hi = int(start_index[c]), int(start_index[c + 1])
    lim = n if call_len is None else min(n, int(call_len))
    out = []
    for i, b in enumerate(seq):
        q = pos + i
        ch = "."
        if i < lim and q < hi:
            g = chr(G[q])
            if conv == "T" and g == "C" and b in "CT":
                meth, q1, q2, key = b == "C", q + 1, q + 2, "G"
            elif conv == "A" and g == "G" and b in "GA":
                meth, q1, q2, key = b == "G", q - 1, q - 2, "C"
            else:
                out.append(ch)
                continue
            if not lo <= q1 < hi:
                k = 3
            elif chr(G[q1]) == key:
                k = 0
            elif not lo <= q2 < hi:
                k = 3
            elif chr(G[q2]) == key:
                k = 1
            else:
                k = 2
            ch = "zxhu"[k]
            if meth:
                ch = ch.upper()
            counts[k + (0 if meth else 4)] += 1
        out.append(ch)
    return "".join(out), counts


def expected_batch(db, seqs, recs, conv, call_len=None, R=None):
    """conv: 'T' / 'A' or a uint8 array.  -> (list of call strings, counts int array [n, 8], totals dict)."""
    R = reference_bases(db) if R is None else R
    calls, counts = [], np.zeros((len(seqs), 8), dtype=np.int64)
    tot = {"reads": 0, "meth": np.zeros(4, dtype=np.int64), "unmeth": np.zeros(4, dtype=np.int64)}
    for i, s in enumerate(seqs):
        cv = conv if isinstance(conv, str) else chr(int(conv[i]))
        c, k = expected_read(R, db.start_index, s, recs["genome_pos"][i], recs["times"][i], bytes(recs["strand"][i]), cv,
                             None if call_len is None else call_len[i])
        calls.append(c)
        counts[i] = k
        if int(recs["times"][i]) == 1 and int(recs["genome_pos"][i]) < db.genome_len and cv in ("T", "A"):
            tot["reads"] += 1
            tot["meth"] += counts[i, :4]
            tot["unmeth"] += counts[i, 4:]
    return calls, counts, tot


def assert_batch(got, seqs, want, what=""):
    """got: (calls, counts, stats) of Index.meth_call_batch; want: expected_batch's.  Every read is compared."""
    calls, counts, stats = got
    wcalls, wcounts, wtot = want
    if calls is not None:
        assert calls.size == sum(len(s) for s in seqs)
        text = calls.tobytes().decode("latin-1")
        at = 0
        for i, s in enumerate(seqs):
            g = text[at:at + len(s)]
            assert g == wcalls[i], "%s read %d calls differ:\n got  %s\n want %s\n read %s" % (what, i, g, wcalls[i], s)
            at += len(s)
    if counts is not None:
        gc = np.concatenate([counts["meth"].astype(np.int64), counts["unmeth"].astype(np.int64)], axis=1)
        bad = np.nonzero((gc != wcounts).any(axis=1))[0]
        assert bad.size == 0, "%s counts differ at %s: got %s want %s" % (what, bad[:5], gc[bad[:5]], wcounts[bad[:5]])
    if stats is not None:
        assert int(stats["reads"][0]) == wtot["reads"], (what, stats, wtot)
        assert np.array_equal(stats["meth"][0].astype(np.int64), wtot["meth"]), (what, stats, wtot)
        assert np.array_equal(stats["unmeth"][0].astype(np.int64), wtot["unmeth"]), (what, stats, wtot)


def load(name):
    names, seqs, scores = [], [], []
    for nm, sq, sc in refio.load_fastq_batches(os.path.join(refio.GOLDEN, name), 10 ** 7):
        names += nm
        seqs += sq
        scores += sc
    return names, seqs, scores


def letters(calls_list):
    return set("".join(calls_list)) - {"."}


# ---------------------------------------------------------------------------
# 1. the golden library
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g1(scratch):
    import walt_amd
    path = os.path.join(scratch, "meth_g1.dbindex")
    walt_amd.makedb(os.path.join(refio.GOLDEN, "g1.fa"), path, threads=4)
    db = refio.DbIndex(path)
    return db, path


@pytest.fixture(scope="module")
def g1_all(g1):
    import walt_amd
    idx = walt_amd.Index.open(g1[1], device=0, strands=walt_amd.STRANDS_ALL | walt_amd.WITH_REFERENCE)
    yield idx
    idx.close()


def test_reference_rule_gives_back_the_fasta(g1):
    db, _ = g1
    fa = "".join(l.strip() for l in open(os.path.join(refio.GOLDEN, "g1.fa")) if not l.startswith(">")).upper()
    R = reference_bases(db)
    assert R[0].tobytes().decode() == fa
    rc = "".join(refio.revcomp(fa[int(db.start_index[c]):int(db.start_index[c + 1])]) for c in range(db.n_chrom))
    assert R[1].tobytes().decode() == rc


def test_golden_se_ct_on_ct_strands_plus_reference(g1):
    import walt_amd
    db, path = g1
    idx = walt_amd.Index.open(path, device=0, strands=walt_amd.STRANDS_CT | walt_amd.WITH_REFERENCE)
    try:
        assert idx.has_reference
        _, seqs, _ = load("se_ct.fastq")
        bases, offs = walt_amd.pack_reads(seqs)
        recs, _ = idx.map_se_batch(bases, offs)
        want = expected_batch(db, seqs, recs, "T")
        assert_batch(idx.meth_call_batch(bases, offs, recs, "T"), seqs, want, "se_ct")
        uniq = recs["times"] == 1
        assert int(uniq.sum()) == 987 and int((recs["strand"][recs["times"] >= 1] == b"-").sum()) == 547
        assert want[2]["reads"] == 987
        assert set("zZxXhHU") <= letters(want[0]), letters(want[0])
    finally:
        idx.close()


def test_golden_se_ga_both_files_cover_all_letters_and_strands(g1):
    import walt_amd
    db, path = g1
    idx = walt_amd.Index.open(path, device=0, strands=walt_amd.STRANDS_GA | walt_amd.WITH_REFERENCE)
    try:
        _, seqs, _ = load("se_ga.fastq")
        bases, offs = walt_amd.pack_reads(seqs)
        recs, _ = idx.map_se_batch(bases, offs, ag_wildcard=True)
        want = expected_batch(db, seqs, recs, "A")
        assert_batch(idx.meth_call_batch(bases, offs, recs, "A"), seqs, want, "se_ga")
        assert int((recs["times"] == 1).sum()) == 484
        assert "".join(want[0]).count("u") == 4
        uniq = recs["times"] == 1
        assert {b"+", b"-"} == set(recs["strand"][uniq].tolist())
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
    want = expected_batch(db, seqs, recs, conv)
    assert_batch(g1_all.meth_call_batch(bases, offs, recs, conv), seqs, want, "mixed -R")
    assert set("zZxXhHuU") <= letters(want[0])


@pytest.mark.parametrize("files", [("pe_1.fastq", "pe_2.fastq"), ("pe150_1.fastq", "pe150_2.fastq")])
def test_golden_pairs_with_stride_64(g1, g1_all, files):
    import walt_amd
    db, _ = g1
    _, s1, _ = load(files[0])
    _, s2, _ = load(files[1])
    b1, o1 = walt_amd.pack_reads(s1)
    b2, o2 = walt_amd.pack_reads(s2)
    out, _ = g1_all.map_pe_batch(b1, o1, b2, o2)
    for seqs, bases, offs, field, cv in ((s1, b1, o1, "m1", "T"), (s2, b2, o2, "m2", "A")):
        recs = out[field]
        assert recs.strides[0] == 64
        want = expected_batch(db, seqs, recs, cv)
        assert_batch(g1_all.meth_call_batch(bases, offs, recs, cv), seqs, want, "%s %s" % (files[0], field))
        if files[0] == "pe_1.fastq":
            assert want[2]["reads"] == (684 if field == "m1" else 685)
            assert set("zZxXhH") <= letters(want[0])


@pytest.mark.parametrize("pattern", [5, 7])
def test_golden_seed_patterns_5_and_7(scratch, pattern):
    import walt_amd
    old = walt_amd.PATTERN
    walt_amd.set_pattern(pattern)
    refio.set_pattern(pattern)
    try:
        path = os.path.join(scratch, "meth_g1_sp%d.dbindex" % pattern)
        walt_amd.makedb(os.path.join(refio.GOLDEN, "g1.fa"), path, threads=4)
        db = refio.DbIndex(path)
        idx = walt_amd.Index.open(path, device=0, strands=walt_amd.STRANDS_ALL | walt_amd.WITH_REFERENCE)
        try:
            for name, ag in (("sp_se_ct.fastq", False), ("sp_se_ga.fastq", True)):
                _, seqs, _ = load(name)
                bases, offs = walt_amd.pack_reads(seqs)
                recs, _ = idx.map_se_batch(bases, offs, ag_wildcard=ag)
                cv = "A" if ag else "T"
                want = expected_batch(db, seqs, recs, cv)
                assert want[2]["reads"] > 0
                assert_batch(idx.meth_call_batch(bases, offs, recs, cv), seqs, want, "pattern %d %s" % (pattern, name))
        finally:
            idx.close()
    finally:
        walt_amd.set_pattern(old)
        refio.set_pattern(3)


# ---------------------------------------------------------------------------
# 2. a planted genome with expected strings written by hand
# ---------------------------------------------------------------------------
def _rnd(rng, n, al="ACGT"):
    return "".join(rng.choice(al) for _ in range(n))


# 60-base cores, each with its expected call string under the conversion named, WRITTEN BY HAND from the table in
# include/walt_amd.h (upper case methylated; z CpG, x CHG, h CHH).  The cores hold no C (or no G) apart from the
# ones listed, so every other position is '.'.
#          0         1         2         3         4         5
#          012345678901234567890123456789012345678901234567890123456789
CORE_T = "ATTAACGATTAACAGTTAACATTAACGTTAACTGATTACAATTAAGTTAAGATTAAGTAA"
#  C at 5 (CG: CpG), 12 (CAG: CHG), 19 (CAT: CHH), 25 (CG: CpG), 31 (CTG: CHG), 38 (CAA: CHH)
READ_T = "ATTAACGATTAATAGTTAACATTAATGTTAACTGATTATAATTAAGTTAAGATTAAGTAA"
#  read: C kept at 5, 19, 31 (methylated); T at 12, 25, 38 (unmethylated)
CALL_T = ".....Z......x......H.....z.....X......h....................."
CORE_A = "TAATTGCTAATTGTCAATTGTAATTGCAATTGACTAATGTTAATTCAATTCTAATTCATT"
#  G at 5: behind it T, A (n1 = G[4] = T, n2 = G[3] = T: CHH); conversion 'A' looks BEHIND: n1 = G[q-1], n2 = G[q-2]
#  G at 5: n1 T, n2 T -> CHH;  G at 12: n1 T, n2 T -> CHH;  G at 19: n1 T n2 T -> CHH; G at 25: n1 T n2 T -> CHH;
#  G at 31: n1 T n2 T -> CHH; G at 38: n1 T, n2 A -> CHH      (the C's ahead of a G do not matter for 'A')
READ_A = "TAATTGCTAATTATCAATTGTAATTACAATTGACTAATATTAATTCAATTCTAATTCATT"
#  read: G kept at 5, 19, 31; A at 12, 25, 38
CALL_A = ".....H......h......H.....h.....H......h....................."
CORE_A2 = "TAACGTTAACTGTAACAGTTACGATTCAGAATTCTGTAATCCGTAATTAATTAATTAATT"
#  G at 4: n1 = C (CpG);  G at 11: n1 = T, n2 = C (CHG);  G at 17: n1 = A, n2 = C (CHG);  G at 22: n1 = C (CpG);
#  G at 28: n1 = A, n2 = C (CHG);  G at 35: n1 = T, n2 = C (CHG);  G at 42: n1 = C (CpG)
READ_A2 = "TAACGTTAACTATAACAGTTACAATTCAGAATTCTATAATCCGTAATTAATTAATTAATT"
#  read: G kept at 4, 17, 28, 42; A at 11, 22, 35
CALL_A2 = "....Z......x.....X....z.....X......x......Z................."


def planted(scratch):
    """chrP1: random flank + cores + flank; chrS: 50 bases (shorter than 64); chrE: starts GGTAGAT, ends TACATCC."""
    rng = random.Random(5)
    cores = [CORE_T, CORE_A, CORE_A2]
    assert all(len(c) == 60 for c in cores)
    flank = lambda n: _rnd(rng, n)
    p1 = flank(400) + CORE_T + flank(300) + CORE_A + flank(300) + CORE_A2 + flank(400)
    short = _rnd(rng, 50)
    body = _rnd(rng, 500)
    chr_e = "GGTAGAT" + body + "TACATCC"
    fa = os.path.join(scratch, "meth_planted.fa")
    with open(fa, "w") as f:
        f.write(">chrP1\n%s\n>chrS\n%s\n>chrE\n%s\n>chrZ\n%s\n" % (p1, short, chr_e, flank(700)))
    return fa, p1, short, chr_e


def _pad_read(core_read, genome, at, left, right, conv):
    """the read = `left` genome bases + core_read + `right` genome bases, the flanks fully converted (unmethylated)"""
    lf, rf = genome[at - left:at], genome[at + len(core_read):at + len(core_read) + right]
    cvt = (lambda s: s.replace("C", "T")) if conv == "T" else (lambda s: s.replace("G", "A"))
    return cvt(lf) + core_read + cvt(rf)


def _flank_calls(R, db, read, pos, conv, left, core_calls, right):
    """hand-written core calls + the restatement for the random flanks (which the other tests cover)"""
    full, _ = expected_read(R, db.start_index, read, pos, 1, b"+", conv)
    return full[:left] + core_calls + full[left + len(core_calls):]


def test_planted_genome_hand_written_calls(scratch):
    import walt_amd
    fa, p1, short, chr_e = planted(scratch)
    path = os.path.join(scratch, "meth_planted.dbindex")
    walt_amd.makedb(fa, path, threads=4)
    db = refio.DbIndex(path)
    R = reference_bases(db)
    idx = walt_amd.Index.open(path, device=0, strands=walt_amd.STRANDS_ALL | walt_amd.WITH_REFERENCE)
    try:
        at_t, at_a, at_a2 = 400, 400 + 60 + 300, 400 + 60 + 300 + 60 + 300
        # --- '+' strand, both conversions: the core's calls are the hand-written strings
        for core_read, calls, at, conv in ((READ_T, CALL_T, at_t, "T"), (READ_A, CALL_A, at_a, "A"),
                                           (READ_A2, CALL_A2, at_a2, "A")):
            read = _pad_read(core_read, p1, at, 20, 20, conv)
            bases, offs = walt_amd.pack_reads([read])
            recs, _ = idx.map_se_batch(bases, offs, ag_wildcard=conv == "A")
            assert int(recs["times"][0]) == 1 and int(recs["genome_pos"][0]) == at - 20 and recs["strand"][0] == b"+"
            got, counts, stats = idx.meth_call_batch(bases, offs, recs, conv)
            text = got.tobytes().decode()
            assert text[20:80] == calls, "\n got  %s\n want %s" % (text[20:80], calls)
            assert text == _flank_calls(R, db, read, at - 20, conv, 20, calls, 20)
            # call_len shorter than the read: everything from there on is '.'
            got2, c2, _ = idx.meth_call_batch(bases, offs, recs, conv, call_len=[45])
            t2 = got2.tobytes().decode()
            assert t2[:45] == text[:45] and t2[45:] == "." * (len(read) - 45)
            assert int(c2["meth"].sum() + c2["unmeth"].sum()) == sum(ch != "." for ch in t2)
        # --- '-' strand: the reverse complement of a read maps on '-' and reads R' left to right.  A G->A read of the
        # forward strand, reverse-complemented, is a C->T read of the reverse strand, with the calls reversed:
        #   forward 'A' call at a G whose context lies BEHIND  ==  reverse 'T' call at the C whose context lies AHEAD
        for core_read, calls, at, conv in ((READ_A2, CALL_A2, at_a2, "A"), (READ_T, CALL_T, at_t, "T")):
            read = _pad_read(core_read, p1, at, 20, 20, conv)
            rc_read = refio.revcomp(read)
            rconv = "T" if conv == "A" else "A"
            bases, offs = walt_amd.pack_reads([rc_read])
            recs, _ = idx.map_se_batch(bases, offs, ag_wildcard=rconv == "A")
            assert int(recs["times"][0]) == 1 and recs["strand"][0] == b"-"
            got, _, _ = idx.meth_call_batch(bases, offs, recs, rconv)
            text = got.tobytes().decode()
            assert text[20:80] == calls[::-1], "\n got  %s\n want %s" % (text[20:80], calls[::-1])
        # --- a mismatch on a C: the read shows A where the reference has C -> no call there
        mm = list(_pad_read(READ_T, p1, at_t, 20, 20, "T"))
        assert mm[20 + 5] == "C"
        mm[20 + 5] = "A"
        bases, offs = walt_amd.pack_reads(["".join(mm)])
        recs, _ = idx.map_se_batch(bases, offs)
        assert int(recs["times"][0]) == 1 and int(recs["mismatch"][0]) == 1
        got, _, _ = idx.meth_call_batch(bases, offs, recs, "T")
        assert got.tobytes().decode()[20:80] == CALL_T[:5] + "." + CALL_T[6:]
        # --- chromosome ends.  chrE = "GGTAGAT" + body + "TACATCC" (expected strings by hand):
        #   end, conversion 'T' (context AHEAD): C at -5: n1 = A, n2 = T -> CHH;  C at -2: n1 = C (inside, not G), n2
        #   outside -> unknown;  C at -1: n1 outside -> unknown
        e0 = int(db.start_index[2])
        e_len = len(chr_e)
        assert chr_e[-7:] == "TACATCC" and chr_e[:7] == "GGTAGAT"

        def call_one(read, conv, want_pos):
            bases, offs = walt_amd.pack_reads([read])
            recs, _ = idx.map_se_batch(bases, offs, ag_wildcard=conv == "A")
            assert int(recs["times"][0]) == 1 and recs["strand"][0] == b"+" and int(recs["genome_pos"][0]) == want_pos, recs
            got, _, _ = idx.meth_call_batch(bases, offs, recs, conv)
            return got.tobytes().decode()

        def call_made_up(read, conv, pos):
            """the mapper never returns a read that reaches its chromosome's last base (mapping.cpp:285 wants one more
            base behind it), so that record is written by hand: the call takes what it is given"""
            bases, offs = walt_amd.pack_reads([read])
            recs = np.zeros(1, dtype=walt_amd.best_match_dtype)
            recs["genome_pos"], recs["times"], recs["strand"] = pos, 1, b"+"
            got, _, _ = idx.meth_call_batch(bases, offs, recs, conv)
            return got.tobytes().decode()

        tail = chr_e[-60:]
        # a read that ends on the chromosome's last base, all three C kept / all three converted
        assert call_made_up(tail[:-7].replace("C", "T") + "TACATCC", "T", e0 + e_len - 60)[-7:] == "..H..UU"
        assert call_made_up(tail[:-7].replace("C", "T") + "TATATTT", "T", e0 + e_len - 60)[-7:] == "..h..uu"
        # ... and one that runs three bases over the end: nothing beyond the chromosome is called
        assert call_made_up(tail[3:-7].replace("C", "T") + "TACATCC" + "CCC", "T", e0 + e_len - 57)[-10:] == "..H..UU..."
        # one that ends one base earlier: its last base is the C at -2 (n1 inside and not G, n2 outside: unknown)
        tail1 = chr_e[-61:-1]
        assert call_one(tail1[:-6].replace("C", "T") + "TACATC", "T", e0 + e_len - 61)[-6:] == "..H..U"
        assert call_one(tail1[:-6].replace("C", "T") + "TATATT", "T", e0 + e_len - 61)[-6:] == "..h..u"
        #   start, conversion 'A' (context BEHIND): G at 0: n1 outside -> unknown;  G at 1: n1 = G (inside, not C), n2
        #   outside -> unknown;  G at 4: n1 = A, n2 = T -> CHH
        head = chr_e[:60]
        assert call_one("GGTAGAT" + head[7:].replace("G", "A"), "A", e0)[:7] == "UU..H.."
        assert call_one("AATAAAT" + head[7:].replace("G", "A"), "A", e0)[:7] == "uu..h.."
        # one that starts at the second base: its first base is the G at 1
        head1 = chr_e[1:61]
        assert call_one("GTAGAT" + head1[6:].replace("G", "A"), "A", e0 + 1)[:6] == "U..H.."
        assert call_one("ATAAAT" + head1[6:].replace("G", "A"), "A", e0 + 1)[:6] == "u..h.."
    finally:
        idx.close()


# ---------------------------------------------------------------------------
# 3. shapes
# ---------------------------------------------------------------------------
def simulated_reads(db, rng, lengths, conv):
    """reads cut from the unconverted '+' reference at random places, partly converted, some with mismatches"""
    R = reference_bases(db)[0].tobytes().decode()
    seqs = []
    for ln in lengths:
        c = rng.randrange(db.n_chrom)
        lo, hi = int(db.start_index[c]), int(db.start_index[c + 1])
        if hi - lo < ln:
            c = int(np.argmax(db.lengths))
            lo, hi = int(db.start_index[c]), int(db.start_index[c + 1])
        at = rng.randrange(lo, hi - ln + 1)
        s = list(R[at:at + ln])
        frm, to = ("C", "T") if conv == "T" else ("G", "A")
        for i, ch in enumerate(s):
            if ch == frm and rng.random() < 0.7:
                s[i] = to
        if rng.random() < 0.3:
            s[rng.randrange(ln)] = rng.choice("ACGT")
        s = "".join(s)
        if rng.random() < 0.5:
            s = refio.revcomp(s)  # the other strand, the other conversion: maps nowhere or anywhere; still compared
        seqs.append(s)
    return seqs


def test_shapes_lengths_alignment_null_outputs_guards(g1, g1_all):
    import walt_amd
    db, _ = g1
    rng = random.Random(77)
    L = walt_amd.lib()
    lo_len = L.walt_min_read_len()
    lengths = [lo_len, lo_len + 1, 47, 63, 64, 65, 100, 101, 127, 128, 129, 150, 255, 256, 257, 500, 777, 1023, 1024]
    lengths += [rng.randrange(lo_len, 300) for _ in range(200)]
    rng.shuffle(lengths)
    R = reference_bases(db)
    for conv in ("T", "A"):
        seqs = simulated_reads(db, rng, lengths, conv)
        bases, offs = walt_amd.pack_reads(seqs)
        assert any(int(o) % 16 for o in offs[1:-1])
        recs, _ = g1_all.map_se_batch(bases, offs, ag_wildcard=conv == "A")
        assert (recs["times"] == 1).sum() > 50
        want = expected_batch(db, seqs, recs, conv, R=R)
        assert_batch(g1_all.meth_call_batch(bases, offs, recs, conv), seqs, want, "shapes " + conv)
        # each output absent in turn
        c, k, s = g1_all.meth_call_batch(bases, offs, recs, conv, want_calls=False)
        assert c is None
        assert_batch((c, k, s), seqs, want)
        c, k, s = g1_all.meth_call_batch(bases, offs, recs, conv, want_counts=False)
        assert k is None
        assert_batch((c, k, s), seqs, want)
        c, k, s = g1_all.meth_call_batch(bases, offs, recs, conv, want_stats=False)
        assert s is None
        assert_batch((c, k, s), seqs, want)
        # two calls accumulate the totals
        _, _, s2 = g1_all.meth_call_batch(bases, offs, recs, conv, stats=s if s is not None else None)
        _, _, s3 = g1_all.meth_call_batch(bases, offs, recs, conv, stats=s2)
        assert int(s3["reads"][0]) == 2 * want[2]["reads"]
        assert np.array_equal(s3["meth"][0].astype(np.int64), 2 * want[2]["meth"])
        # n = 1 and n = 0
        one = g1_all.meth_call_batch(*walt_amd.pack_reads(seqs[:1]), recs[:1], conv)
        assert_batch(one, seqs[:1], expected_batch(db, seqs[:1], recs[:1], conv, R=R))
        c0, k0, s0 = g1_all.meth_call_batch(np.zeros(0, np.uint8), np.zeros(1, np.uint64), recs[:0], conv)
        assert c0.size == 0 and k0.size == 0 and int(s0["reads"][0]) == 0
        # a slice of the batch through offsets that do not start at 0, and the bytes around its calls stay untouched
        lo_r, hi_r = 7, 60
        n = hi_r - lo_r
        total = int(offs[-1])
        calls = np.full(total + 2, 0x23, dtype=np.uint8)  # '#' guards before, after and around the slice
        counts = np.zeros(n, dtype=walt_amd.meth_counts_dtype)
        sub_offs = np.ascontiguousarray(offs[lo_r:hi_r + 1])
        sub_recs = np.ascontiguousarray(recs[lo_r:hi_r])
        rc = L.walt_meth_call_batch(g1_all.handle, bases.ctypes.data, sub_offs.ctypes.data, n, sub_recs.ctypes.data, 16,
                                    None, 0, ord(conv), None, calls.ctypes.data + 1, counts.ctypes.data, None)
        assert rc == 0, L.walt_last_error()
        a, b = int(offs[lo_r]), int(offs[hi_r])
        assert (calls[:1 + a] == 0x23).all() and (calls[1 + b:] == 0x23).all()
        assert calls[1 + a:1 + b].tobytes().decode() == "".join(want[0][lo_r:hi_r])


# ---------------------------------------------------------------------------
# 4. index forms
# ---------------------------------------------------------------------------
def test_index_forms(g1, g1_all):
    import walt_amd
    db, path = g1
    _, seqs, _ = load("se_ct.fastq")
    bases, offs = walt_amd.pack_reads(seqs)
    recs, _ = g1_all.map_se_batch(bases, offs)
    ref_calls = g1_all.meth_call_batch(bases, offs, recs, "T")
    # from_host with four strands: no reference until enable_reference
    fh = walt_amd.Index.from_host(db.lengths, db.genome, db.counter, db.index, chrom_names=db.names)
    try:
        assert not fh.has_reference
        with pytest.raises(walt_amd.WaltError) as ei:
            fh.meth_call_batch(bases, offs, recs, "T")
        assert ei.value.code == walt_amd.WALT_EINVAL and "reference" in str(ei.value)
        before = fh.device_bytes
        fh.enable_reference()
        assert fh.has_reference
        after = fh.device_bytes
        assert db.genome_len // 2 <= after - before < db.genome_len
        fh.enable_reference()
        assert fh.device_bytes == after
        got = fh.meth_call_batch(bases, offs, recs, "T")
        assert np.array_equal(got[0], ref_calls[0]) and np.array_equal(got[1], ref_calls[1])
        assert got[2].tobytes() == ref_calls[2].tobytes()
    finally:
        fh.close()
    # C->T strands only, without the bit: no reference, EINVAL from the call and from enable_reference
    ct = walt_amd.Index.open(path, device=0, strands=walt_amd.STRANDS_CT)
    ctr = walt_amd.Index.open(path, device=0, strands=walt_amd.STRANDS_CT | walt_amd.WITH_REFERENCE)
    try:
        assert not ct.has_reference and ctr.has_reference
        with pytest.raises(walt_amd.WaltError) as ei:
            ct.meth_call_batch(bases, offs, recs, "T")
        assert ei.value.code == walt_amd.WALT_EINVAL and "reference" in str(ei.value)
        with pytest.raises(walt_amd.WaltError) as ei:
            ct.enable_reference()
        assert ei.value.code == walt_amd.WALT_EINVAL and "GA10" in str(ei.value) and "GA11" in str(ei.value)
        extra = ctr.device_bytes - ct.device_bytes
        assert db.genome_len // 2 <= extra < db.genome_len, extra
        got = ctr.meth_call_batch(bases, offs, recs, "T")
        assert np.array_equal(got[0], ref_calls[0])
        # argument errors name their cause
        L = walt_amd.lib()
        rc = L.walt_meth_call_batch(ctr.handle, bases.ctypes.data, offs.ctypes.data, len(seqs), recs.ctypes.data, 8, None, 0,
                                    ord("T"), None, None, None, None)
        assert rc == walt_amd.WALT_EINVAL and b"stride" in L.walt_last_error()
        rc = L.walt_meth_call_batch(ctr.handle, bases.ctypes.data, offs.ctypes.data, len(seqs), recs.ctypes.data, 16, None, 0,
                                    ord("X"), None, None, None, None)
        assert rc == walt_amd.WALT_EINVAL and b"neither 'T' nor 'A'" in L.walt_last_error()
        bad_conv = np.full(len(seqs), ord("T"), dtype=np.uint8)
        bad_conv[3] = ord("C")
        with pytest.raises(walt_amd.WaltError) as ei:
            ctr.meth_call_batch(bases, offs, recs, bad_conv)
        assert ei.value.code == walt_amd.WALT_EINVAL and "neither" in str(ei.value)
    finally:
        ct.close()
        ctr.close()


def test_fasta_with_a_run_of_n(scratch):
    """Where the FASTA had N each strand file holds its own fill; the calls equal the rule on the files as written."""
    import walt_amd
    rng = random.Random(9)
    a, b = _rnd(rng, 3000), _rnd(rng, 3000)
    fa = os.path.join(scratch, "meth_n.fa")
    with open(fa, "w") as f:
        f.write(">n1\n%s%s%s\n>n2\n%s\n" % (a, "N" * 40, b, _rnd(rng, 1500)))
    path = os.path.join(scratch, "meth_n.dbindex")
    walt_amd.makedb(fa, path, threads=4)
    db = refio.DbIndex(path)
    idx = walt_amd.Index.open(path, device=0, strands=walt_amd.STRANDS_CT | walt_amd.WITH_REFERENCE)
    try:
        # reads that run into the N run from both sides (their N-side bases are whatever: up to 6 mismatches map)
        seqs = []
        for k in (0, 2, 4, 6):
            seqs.append(a[-(100 - k):].replace("C", "T") + _rnd(rng, k, "AT"))
            seqs.append(_rnd(rng, k, "AT") + b[:100 - k].replace("C", "T"))
        bases, offs = walt_amd.pack_reads(seqs)
        recs, _ = idx.map_se_batch(bases, offs)
        assert (recs["times"] == 1).sum() >= 4
        assert_batch(idx.meth_call_batch(bases, offs, recs, "T"), seqs, expected_batch(db, seqs, recs, "T"), "N run")
    finally:
        idx.close()


# ---------------------------------------------------------------------------
# 5. device form
# ---------------------------------------------------------------------------
def test_device_form_on_a_stream_and_made_up_records(g1, g1_all):
    import torch
    import walt_amd
    db, _ = g1
    _, seqs, _ = load("se_ct.fastq")
    bases, offs = walt_amd.pack_reads(seqs)
    recs, _ = g1_all.map_se_batch(bases, offs)
    recs = recs.copy()
    # made-up records: positions at and beyond the genome's end are treated as unmapped
    recs["genome_pos"][5] = db.genome_len
    recs["genome_pos"][6] = 0xFFFFFFF0
    recs["times"][5] = recs["times"][6] = 1
    n = len(seqs)
    host = g1_all.meth_call_batch(bases, offs, recs, "T")
    want = expected_batch(db, seqs, recs, "T")
    assert want[0][5] == "." * len(seqs[5]) and want[0][6] == "." * len(seqs[6])
    assert_batch(host, seqs, want, "host form, made-up records")
    dev = torch.device("cuda", 0)
    d_bases = torch.from_numpy(bases).to(dev)
    d_offs = torch.from_numpy(offs.view(np.int64)).to(dev)
    d_recs = torch.from_numpy(recs.view(np.uint8).reshape(n, 16)).to(dev)
    d_calls = torch.full((bases.size + 32,), 0x23, dtype=torch.uint8, device=dev)
    d_counts = torch.zeros((n, 16), dtype=torch.uint8, device=dev)
    d_stats = torch.zeros(9, dtype=torch.int64, device=dev)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    for shift in (16, 3):  # the calls array aligned like the bases, and not
        d_stats.zero_()
        d_calls.fill_(0x23)
        stream.wait_stream(torch.cuda.current_stream())
        g1_all.meth_call_batch_device(d_bases.data_ptr(), d_offs.data_ptr(), n, d_recs.data_ptr(), 16, None, 1, "T", None,
                                      d_calls.data_ptr() + shift, d_counts.data_ptr(), d_stats.data_ptr(),
                                      stream=stream.cuda_stream)
        stream.synchronize()
        calls = d_calls.cpu().numpy()
        total = int(offs[-1])
        assert (calls[:shift] == 0x23).all() and (calls[shift + total:] == 0x23).all()
        assert np.array_equal(calls[shift:shift + total], host[0])
        assert d_counts.cpu().numpy().tobytes() == host[1].tobytes()
        assert d_stats.cpu().numpy().tobytes() == host[2].tobytes()


# ---------------------------------------------------------------------------
# 6. command line
# ---------------------------------------------------------------------------
def run_walt(args, timeout=600):
    pr = subprocess.run([WALT_BIN] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
    assert pr.returncode == 0, pr.stdout[-2000:]
    return pr.stdout


def strip_xm(line):
    parts = line.rstrip("\n").split("\t")
    xm = [p for p in parts if p.startswith("XM:Z:")]
    rest = [p for p in parts if not p.startswith("XM:Z:")]
    assert len(xm) <= 1
    return "\t".join(rest) + "\n", (xm[0][5:] if xm else None)


def methstats_text(blocks):
    out = []
    for head, tot in blocks:
        if head:
            out.append(head + "\n")
        out.append("reads\t%d\n" % tot["reads"])
        for k, name in enumerate(CONTEXTS):
            m, u = int(tot["meth"][k]), int(tot["unmeth"][k])
            out.append("%s\t%d\t%d\t%s\n" % (name, m, u, "%.6f" % (m / (m + u)) if m + u else "NA"))
    return "".join(out)


def clip_point(adaptor, s):
    """where refio.clip_adaptor (util.hpp:202-216) starts to write N; len(s) when it clips nothing"""
    n = len(s)
    lim1 = max(n - 14 + 1, 0)
    for i in range(lim1):
        if refio._similarity(s, i, adaptor) >= 11:
            return i
    for i in range(lim1, n - 5 + 1):
        if refio._similarity(s, i, adaptor) >= n - i - 1:
            return i
    return n


def cli_records_se(idx, seqs, mode):
    import walt_amd
    bases, offs = walt_amd.pack_reads(seqs)
    if mode == "R":
        recs, conv, _ = idx.map_se_rpbat_batch(bases, offs)
        return recs, conv
    recs, _ = idx.map_se_batch(bases, offs, ag_wildcard=mode == "A")
    return recs, "A" if mode == "A" else "T"


@pytest.mark.parametrize("case", ["se_ct", "se_ga_A", "mixed_R", "se_clip_C"])
def test_cli_single_end(g1, g1_all, scratch, case):
    from test_gpu_rpbat import mixed_library
    db, path = g1
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
        fq = os.path.join(scratch, "meth_mixed.fastq")
        with open(fq, "w") as f:
            for nm, s, q in zip(names, seqs, scores):
                f.write("@%s\n%s\n+\n%s\n" % (nm, s, q))
        extra, mode = ["-R"], "R"
    outs = {}
    for tag, more in (("plain", []), ("meth", ["-M"]), ("mr_plain", None), ("mr_meth", None), ("g00", ["-M", "-g", "0,0"])):
        out = os.path.join(scratch, "meth_cli_%s_%s.out" % (case, tag))
        if more is None:
            run_walt(["-i", path, "-r", fq, "-o", out, "-a", "-u"] + extra + (["-M"] if tag == "mr_meth" else []))
        else:
            run_walt(["-i", path, "-r", fq, "-o", out, "-sam", "-a", "-u"] + extra + more)
        outs[tag] = out
    assert not os.path.exists(outs["plain"] + ".methstats") and not os.path.exists(outs["mr_plain"] + ".methstats")
    plain = open(outs["plain"]).readlines()
    meth = open(outs["meth"]).readlines()
    assert "XM:Z:" not in "".join(plain)
    assert len(plain) == len(meth)
    # expected calls: the loader's reads (clipped and N-filled as the run saw them) are the SEQ fields of the plain run
    call_len = []
    raw = [l.split("\t") for l in plain if not l.startswith("@")]
    rows = [l for l in meth if not l.startswith("@")]
    loaded = []
    for nm, sq, sc in refio.load_fastq_batches(fq, 10 ** 7, adaptor):
        loaded += sq
    assert len(loaded) == len(raw)
    if adaptor:
        raw_reads = [l.rstrip(b"\n") for l in open(fq, "rb").readlines()[1::4]]
        assert len(raw_reads) == len(loaded)
        call_len = [clip_point(adaptor.encode(), bytearray(r)) for r in raw_reads]
        assert sum(c < len(r) for c, r in zip(call_len, raw_reads)) > 10
    recs, conv = cli_records_se(g1_all, loaded, mode)
    want = expected_batch(db, loaded, recs, conv, call_len or None)
    n_xm = 0
    for i, (pl, ml) in enumerate(zip([l for l in plain if not l.startswith("@")], rows)):
        stripped, xm = strip_xm(ml)
        assert stripped == pl, (i, ml, pl)
        mapped = int(recs["times"][i]) >= 1
        assert (xm is not None) == mapped, (i, ml)
        if mapped:
            n_xm += 1
            exp = want[0][i][::-1] if bytes(recs["strand"][i]) == b"-" else want[0][i]
            assert xm == exp, "read %d\n got  %s\n want %s" % (i, xm, exp)
            if adaptor:
                seq_order = xm[::-1] if bytes(recs["strand"][i]) == b"-" else xm
                assert set(seq_order[call_len[i]:]) <= {"."}
    assert n_xm > 100
    stats_text = methstats_text([(None, want[2])])
    assert open(outs["meth"] + ".methstats").read() == stats_text
    assert open(outs["mr_meth"] + ".methstats").read() == stats_text
    assert open(outs["mr_meth"], "rb").read() == open(outs["mr_plain"], "rb").read()
    for sfx in ("", ".methstats", ".mapstats"):
        assert open(outs["g00"] + sfx, "rb").read() == open(outs["meth"] + sfx, "rb").read(), sfx


def test_cli_paired_end(g1, g1_all, scratch):
    import walt_amd
    db, path = g1
    f1, f2 = os.path.join(refio.GOLDEN, "pe_1.fastq"), os.path.join(refio.GOLDEN, "pe_2.fastq")
    outs = {}
    for tag, more in (("plain", ["-sam"]), ("meth", ["-sam", "-M"]), ("mr_plain", []), ("mr_meth", ["-M"]),
                      ("g00", ["-sam", "-M", "-g", "0,0"])):
        out = os.path.join(scratch, "meth_cli_pe_%s.out" % tag)
        run_walt(["-i", path, "-1", f1, "-2", f2, "-o", out, "-a", "-u"] + more)
        outs[tag] = out
    _, s1, _ = load("pe_1.fastq")
    _, s2, _ = load("pe_2.fastq")
    b1, o1 = walt_amd.pack_reads(s1)
    b2, o2 = walt_amd.pack_reads(s2)
    res, _ = g1_all.map_pe_batch(b1, o1, b2, o2)
    w1 = expected_batch(db, s1, res["m1"], "T")
    w2 = expected_batch(db, s2, res["m2"], "A")
    plain = [l for l in open(outs["plain"]) if not l.startswith("@")]
    meth = [l for l in open(outs["meth"]) if not l.startswith("@")]
    assert len(plain) == len(meth) == 2 * len(s1)
    n_xm = 0
    for k, (pl, ml) in enumerate(zip(plain, meth)):
        stripped, xm = strip_xm(ml)
        assert stripped == pl
        i, mate = k // 2, k % 2
        rec = res["m2" if mate else "m1"][i]
        want = (w2 if mate else w1)[0][i]
        assert (xm is not None) == (int(rec["times"]) >= 1), ml
        if xm is not None:
            n_xm += 1
            assert xm == (want[::-1] if bytes(rec["strand"]) == b"-" else want), (k, ml)
    assert n_xm > 1000
    stats_text = methstats_text([("mate1", w1[2]), ("mate2", w2[2])])
    assert open(outs["meth"] + ".methstats").read() == stats_text
    assert open(outs["mr_meth"] + ".methstats").read() == stats_text
    assert open(outs["mr_meth"], "rb").read() == open(outs["mr_plain"], "rb").read()
    assert not os.path.exists(outs["plain"] + ".methstats")
    for sfx in ("", ".methstats", ".mapstats"):
        assert open(outs["g00"] + sfx, "rb").read() == open(outs["meth"] + sfx, "rb").read(), sfx
