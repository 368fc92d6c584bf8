"""Genomes and reads for the tests of the grouped dense verifier (map_se.hip k_se_verify_shared) -- pure Python, no
device: tests/test_share_inputs_cpu.py proves on the host that the inputs are decisive, tests/test_gpu_verify_share_edges.py
maps them.

ENDS GENOME.  k_se_verify_shared applies the sequence-bounds test `pos - c_lo >= seed_i && g + len < c_hi` per read of a
unit, on bounds computed once per record.  On a dense record only the left term can fail, so the edge is a repeat copy
within kPat - 1 bases of the START of its sequence, on either strand.  A family is one motif M of 130 random bases; a
copy's sequence is P[-k:] + M + 230 random bases + P with the pad P = "GATCAGT" and the lead k cycling through LEADS,
and the second half of a family's copies is written reverse-complemented as a whole: there the copy lies at the END of
its FASTA sequence and at the start of it on the reverse strand.  File order: a 3,000-base flank that ends in P, the
forward sequences (shuffled), optional unrelated filler sequences that begin with revcomp(P) and end with P, the
reverse-complemented sequences (shuffled), a flank that begins with revcomp(P) -- so whatever precedes a copy on
either strand ends in P, and a read P[-s:] + M[:L - s] occurs EXACTLY in the concatenated strand genome at every copy
with lead 0 (and, by the C->T conversion of the pad, at others), across the border of two sequences.  The reference
rejects those alignments (the read would start in another sequence); a verifier that applies another read's seed
shift, or none, counts them, and the record's `times` differs.

LONG LADDER.  tests/test_gpu_verify_share.py's world with a 130-base motif, for reads of 113 to 128 bases (a 128-base
read's seed spans 126 bases plus the shift, and a region is the candidates equal in all of them)."""
import random

import numpy as np

import refio

PAD = "GATCAGT"
MOTIF = 130
TAIL = 230
FLANK = 3000
N_BACKGROUND = 300
# read lengths of one batch, per seed pattern: reads of up to 112 bases take the 7-word kernel instance, of 113 to 128
# the 8-word one; pattern 5 groups at 7 words only (its 8-word instance has seeds beyond the key), pattern 7 never
ENDS_LENGTHS = {3: [(100, 104, 112), (113, 120, 128), (100, 112, 113, 128)], 5: [(100, 112), (119, 128)], 7: [(100,)]}
COPIES = 9  # reads per (family, shift, length): 2 R + 1 for units of R = 4 items -- two units and part of a third

meta_dtype = np.dtype([("family", "<i4"), ("shift", "<i4"), ("length", "<i4"), ("plain", "?")])


def rand(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def convert(rng, s, ag, rate=0.95):
    a, b = ("G", "A") if ag else ("C", "T")
    return "".join(b if (c == a and rng.random() < rate) else c for c in s)


def substitute(rng, s, k, lo=0, period=1):
    """k substitutions at offsets >= lo.  period = kPat: all at offsets of ONE residue modulo the seed pattern's period,
    so that some seed shift cares about none of them and the read maps whatever k is (three substitutions of three
    residues break every seed of pattern 3)"""
    s = list(s)
    c = rng.randrange(period)
    for p in rng.sample([p for p in range(lo, len(s)) if p % period == c], k):
        s[p] = rng.choice([c for c in "ACGT" if c != s[p]])
    return "".join(s)


def leads_of(pattern):
    """leads of the copies: every seed shift 0 .. kPat - 1 has copies it fits and copies it does not"""
    return tuple(range(7)) if pattern == 7 else (0, 1, 2, 3, 4, 6)


def ends_genome(pattern, per_strand=(20, 66, 130), fillers=0):
    """-> {"pattern", "seqs": [(name, text)], "motifs": [M per family], "flanks": (left, right), "leads": {name: lead}}.
    per_strand: copies of a family on either strand -- one partial 64-record step of at least kWinMinRun = 17 slots, one
    step plus two, two steps plus two.  fillers = 0: 434 sequences (the verifier's LDS table of sequence starts);
    fillers = 700: more than 1,023 (walt::chrom_bounds)."""
    rng = random.Random(1000 * pattern + fillers + 17)
    leads = leads_of(pattern)
    motifs, fwd, rev = [], [], []
    for N in per_strand:
        M = rand(rng, MOTIF)
        motifs.append(M)
        for i in range(2 * N):
            k = leads[i % len(leads)]
            text = (PAD[-k:] if k else "") + M + rand(rng, TAIL) + PAD
            if i < N:
                fwd.append((k, text))
            else:
                rev.append((k, refio.revcomp(text)))
    rng.shuffle(fwd)
    rng.shuffle(rev)
    left = rand(rng, FLANK - len(PAD)) + PAD
    right = refio.revcomp(PAD) + rand(rng, FLANK - len(PAD))
    fill = [refio.revcomp(PAD) + rand(rng, rng.randint(60, 200) - 2 * len(PAD)) + PAD for _ in range(fillers)]
    seqs = [("left", left)] + [("f%d" % i, t) for i, (_, t) in enumerate(fwd)] + [("x%d" % i, t) for i, t in enumerate(fill)]
    seqs += [("r%d" % i, t) for i, (_, t) in enumerate(rev)] + [("right", right)]
    lead = {"f%d" % i: k for i, (k, _) in enumerate(fwd)}
    lead.update({"r%d" % i: k for i, (k, _) in enumerate(rev)})
    return {"pattern": pattern, "fillers": fillers, "seqs": seqs, "motifs": motifs, "flanks": (left, right), "leads": lead}


def write_fasta(seqs, path):
    with open(path, "w") as f:
        for nm, s in seqs:
            f.write(">%s\n%s\n" % (nm, s))


def ends_reads(rng, genome, lengths, copies=COPIES, ag=False):
    """For every family, every shift s in 0 .. kPat - 1 and every length L: `copies` reads P[-s:] + M[:L - s] -- the first
    fully converted and unsubstituted, the others with random conversion and 0 .. 3 substitutions at offsets >= s (the
    pad stays exact) of one residue modulo kPat (substitute), a quarter of them reverse-complemented -- and 300 unique background reads from the two flanks;
    shuffled, so that shifts and lengths mix within a unit.  -> (reads, meta[meta_dtype]); family -1: background."""
    assert copies >= 9
    reads, meta = [], []
    for f, M in enumerate(genome["motifs"]):
        for s in range(genome["pattern"]):
            for L in lengths:
                text = (PAD[-s:] if s else "") + M[:L - s]
                assert len(text) == L
                reads.append(convert(rng, text, ag, rate=1.0))
                meta.append((f, s, L, True))
                for _ in range(copies - 1):
                    t = substitute(rng, text, rng.choice([0, 1, 1, 2, 2, 3]), lo=s, period=genome["pattern"])
                    # (at the largest lead the other strand's alignment ends ON the sequence's end, and the reference asks for
                    # genome_pos + length < end: such a read would map nowhere -- pattern 7's shift 6 only)
                    if s < max(genome["leads"].values()) and rng.random() < 0.25:
                        t = refio.revcomp(t)
                    reads.append(convert(rng, t, ag))
                    meta.append((f, s, L, False))
    for i in range(N_BACKGROUND):
        g = genome["flanks"][i % 2]
        L = rng.choice(lengths)
        p = rng.randrange(10, len(g) - L - 10)
        frag = g[p:p + L]
        frag = refio.revcomp(frag) if rng.random() < 0.5 else frag
        reads.append(substitute(rng, convert(rng, frag, ag), rng.choice([0, 1, 2, 3])))
        meta.append((-1, 0, L, False))
    order = list(range(len(reads)))
    rng.shuffle(order)
    return [reads[i] for i in order], np.array([meta[i] for i in order], dtype=meta_dtype)


def ends_pool(genome, lengths, ag=False):
    """the batch of `lengths` on this genome, the same wherever it is built"""
    seed = 7919 * genome["pattern"] + genome["fillers"] + 31 * sum(lengths) + len(lengths) + (5 if ag else 0)
    return ends_reads(random.Random(seed), genome, lengths, COPIES, ag)


def assert_decisive(db, reads, meta, want, ag=False, what=""):
    """The oracle's records `want` depend on the per-read bounds test: for every family, every shift s > 0 and every
    length, the unsubstituted read's `times` is smaller than at s = 0 and smaller than the number of its exact
    occurrences in the two concatenated strand genomes (which ignores sequence ends).  And the batch is a fair one: at
    least 0.8 of its reads map, every family read more than once."""
    genomes = [bytes(db.genome[s]) for s in ((2, 3) if ag else (0, 1))]
    times = want["times"].astype(np.int64)
    plain = np.flatnonzero(meta["plain"])
    at0 = {(int(meta["family"][i]), int(meta["length"][i])): int(times[i]) for i in plain if meta["shift"][i] == 0}
    checked = 0
    for i in plain:
        f, s, L = int(meta["family"][i]), int(meta["shift"][i]), int(meta["length"][i])
        assert int(want["mismatch"][i]) == 0, "%s family %d shift %d length %d: %d mismatches" % (what, f, s, L, want["mismatch"][i])
        if s == 0:
            continue
        exact = sum(g.count(reads[i].encode()) for g in genomes)
        assert times[i] < at0[(f, L)], "%s family %d length %d: times %d at shift %d, %d at shift 0" % (what, f, L, times[i], s, at0[(f, L)])
        assert times[i] < exact, "%s family %d shift %d length %d: times %d, exact occurrences %d" % (what, f, s, L, times[i], exact)
        checked += 1
    assert checked == int(meta["shift"].max()) * len(at0) > 0  # every (family, length) at every shift 1 .. kPat - 1
    assert (times > 0).mean() >= 0.8, "%s: %.2f of the reads map" % (what, (times > 0).mean())
    fam = meta["family"] >= 0
    assert (times[fam] > 1).all(), "%s: family reads with times <= 1: %s" % (what, np.flatnonzero(fam & (times <= 1))[:8])


# ---------------------------------------------------------------------------------------------------------------
# the long ladder
# ---------------------------------------------------------------------------------------------------------------
LADDER_SPACER = 20
LADDER_FAMILIES = [34, 130, 258, 2050]  # 2,050: 1,025 candidates per strand, just past kBigFirst = 1,024
LADDER_LENGTHS = (113, 120, 128)
LADDER_BACKGROUND = 2000
LADDER_FLANK = 30000


def long_ladder():
    """-> (sequences, copies): every family N identical 130-base motifs with 20-base random spacers, every second copy
    reverse-complemented, shuffled over three sequences between 30,000-base flanks; copies = (sequence number, start,
    family, reverse-complemented)"""
    rng = random.Random(4712)
    units = []
    for N in LADDER_FAMILIES:
        motif = rand(rng, MOTIF)
        units += [(N, motif + rand(rng, LADDER_SPACER), k % 2 == 1) for k in range(N)]
    rng.shuffle(units)
    seqs, copies = [], []
    per = (len(units) + 2) // 3
    for s in range(3):
        parts, pos = [rand(rng, LADDER_FLANK)], LADDER_FLANK
        for fam, text, rc in units[s * per:(s + 1) * per]:
            copies.append((s, pos, fam, rc))
            parts.append(refio.revcomp(text) if rc else text)
            pos += len(text)
        parts.append(rand(rng, LADDER_FLANK))
        seqs.append(("long%d" % s, "".join(parts)))
    return seqs, copies


def ladder_read(rng, seqs, copy, L):
    """a read that meets the copy's motif at seed 0, 1 or 2, from either strand, converted, with 0 .. 3 substitutions"""
    s, pos, fam, rc = copy
    g = seqs[s][1]
    off = rng.choice([0, 1, 2])
    if rc:  # the motif's first base is the unit's last: the read is taken from the other strand
        end = pos + MOTIF + LADDER_SPACER + off
        frag = refio.revcomp(g[end - L:end])
    else:
        frag = g[pos - off:pos - off + L]
    assert len(frag) == L
    if rng.random() < 0.15:
        frag = refio.revcomp(frag)
    return substitute(rng, convert(rng, frag, False), rng.choice([0, 1, 1, 2, 2, 3]))


def ladder_pool(seqs, copies, per_family=130):
    """-> (reads, family): per_family reads of every family -- the first two MADE for one region (two forward copies,
    128 bases, seed shift 0, fully converted, unsubstituted), the others over the three lengths, seed shifts, strands
    and substitutions -- and 2,000 unique background reads (family 0)"""
    rng = random.Random(4713)
    reads, family = [], []
    for N in LADDER_FAMILIES:
        mine = [c for c in copies if c[2] == N]
        for s_, pos, _, _ in [c for c in mine if not c[3]][:2]:
            reads.append(convert(rng, seqs[s_][1][pos:pos + 128], False, rate=1.0))
            family.append(N)
        for _ in range(per_family - 2):
            reads.append(ladder_read(rng, seqs, rng.choice(mine), rng.choice(LADDER_LENGTHS)))
            family.append(N)
    for _ in range(LADDER_BACKGROUND):
        nm, g = seqs[rng.randrange(3)]
        L = rng.choice(LADDER_LENGTHS)
        p = rng.choice([rng.randrange(0, LADDER_FLANK - L), len(g) - LADDER_FLANK + rng.randrange(0, LADDER_FLANK - L)])
        frag = g[p:p + L]
        frag = refio.revcomp(frag) if rng.random() < 0.5 else frag
        reads.append(substitute(rng, convert(rng, frag, False), rng.choice([0, 1, 2, 3])))
        family.append(0)
    return reads, np.array(family)


def ladder_batch(family, m):
    """m reads of every family (the pool's first m of each) and every background read, shuffled the same way every time"""
    sel = np.concatenate([np.flatnonzero(family == N)[:m] for N in LADDER_FAMILIES] + [np.flatnonzero(family == 0)])
    return np.random.RandomState(m).permutation(sel)
