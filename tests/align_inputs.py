"""Reads for tests/test_gpu_verify_align.py on the ends genome of tests/share_inputs.py (families of 20, 66 and 130 copies
per strand: one 64-record step, one step plus two candidates, three steps) -- pure Python, no device;
tests/test_align_inputs_cpu.py proves on the host that they are decisive.

The dense verifiers compare a read with the record's words as they lie (core.h count_mismatch_aligned): the read's last
bases may fall into the word behind the record's NW, which is compared only when the read reaches it (`top`).  So every
(family, lead, length) has nine reads -- full units of four, a unit of one, every seed shift among them -- with the
substitutions where a dropped or doubled word edge shows: the read's first base, its last base, its last-but-one base.
A substitution is always a mismatch under the C->T rule (A <-> G, or A / G for C and T) and is made after the
conversion.  `last_restored` is the same batch with every substituted LAST base put back: the record of a read whose
last base is ignored."""
import random

import numpy as np

import refio
import share_inputs as si

# batches by kernel instance: 7 words on dense records (up to kWinMaxLen1 = 110 bases for seed pattern 3), 7 words on the
# gather route (111, 112), 8 words (at seed shift 0 the bases 127 and 128 lie in the ninth record word)
LENGTHS = [(100, 109, 110), (111, 112), (113, 126, 127, 128)]
COPIES = 9
N_BACKGROUND = 300

meta_dtype = np.dtype([("family", "<i4"), ("lead", "<i4"), ("length", "<i4"), ("kind", "<i4")])
PLAIN, FIRST, LAST, LAST_BUT_ONE, LAST_TWO, RANDOM = range(6)


def mismatching(base):
    return {"A": "G", "G": "A"}.get(base, "A")


def put(text, at):
    t = list(text)
    for p in at:
        t[p] = mismatching(t[p])
    return "".join(t)


def pool(genome, lengths):
    """-> (reads, last_restored, meta[meta_dtype]); family -1: background reads from the flanks"""
    rng = random.Random(104729 + 131 * sum(lengths) + len(lengths))
    reads, restored, meta = [], [], []
    for f, M in enumerate(genome["motifs"]):
        for s in range(genome["pattern"]):
            for L in lengths:
                text = si.convert(rng, (si.PAD[-s:] if s else "") + M[:L - s], False, rate=1.0)
                assert len(text) == L
                for kind, at in ((PLAIN, ()), (FIRST, (0,)), (LAST, (L - 1,)), (LAST_BUT_ONE, (L - 2,)), (LAST_TWO, (L - 2, L - 1)),
                                 (LAST, (L - 1,)), (LAST, (L - 1, 40 + s)), (RANDOM, None), (RANDOM, None)):
                    if at is None:
                        t = si.substitute(rng, text, rng.choice([1, 2, 3]), lo=s, period=genome["pattern"])
                        t = r = si.convert(rng, t, False, rate=1.0)
                    else:
                        t = put(text, at)
                        r = put(text, [p for p in at if p != L - 1])
                    reads.append(t)
                    restored.append(r)
                    meta.append((f, s, L, kind))
    for i in range(N_BACKGROUND):
        g = genome["flanks"][i % 2]
        L = rng.choice(lengths)
        p = rng.randrange(10, len(g) - L - 10)
        frag = g[p:p + L]
        frag = refio.revcomp(frag) if rng.random() < 0.5 else frag
        t = si.substitute(rng, si.convert(rng, frag, False), rng.choice([0, 1, 2, 3]))
        reads.append(t)
        restored.append(t)
        meta.append((-1, 0, L, RANDOM))
    order = list(range(len(reads)))
    rng.shuffle(order)
    return [reads[i] for i in order], [restored[i] for i in order], np.array([meta[i] for i in order], dtype=meta_dtype)


def assert_decisive(want, want_restored, meta, what=""):
    """For every (length, lead) at least one read's record changes when its last base is ignored -- and in fact every
    read whose last base alone was substituted maps with exactly that one mismatch; the family reads map."""
    fam = meta["family"] >= 0
    assert (want["times"][fam] > 0).all(), "%s: family reads that do not map: %s" % (what, np.flatnonzero(fam & (want["times"] == 0))[:8])
    differs = (want["mismatch"] != want_restored["mismatch"]) | (want["times"] != want_restored["times"]) | (want["genome_pos"] != want_restored["genome_pos"])
    for L in sorted(set(int(v) for v in meta["length"][fam])):
        for s in sorted(set(int(v) for v in meta["lead"][fam])):
            sel = fam & (meta["length"] == L) & (meta["lead"] == s)
            assert differs[sel].any(), "%s length %d lead %d: no record depends on the read's last base" % (what, L, s)
    only_last = fam & (meta["kind"] == LAST)
    assert (want["mismatch"][only_last] == want_restored["mismatch"][only_last] + 1).all()
    assert not differs[~fam].any()


def pairs(genome, lengths, n=600):
    """Pairs inside single forward sequences of the families: mate 1 begins at the copy's motif (the family's region, a
    dense item of the paired-end verifier) less 0 .. lead bases, mate 2 ends the fragment in the copy's own random tail;
    a third of the first mates with their last base substituted, a third with the last but one.  -> (mates 1, mates 2)"""
    rng = random.Random(15485863 + sum(lengths))
    fwd = [(nm, text) for nm, text in genome["seqs"] if nm.startswith("f")]
    s1, s2 = [], []
    while len(s1) < n:
        nm, text = rng.choice(fwd)
        lead = genome["leads"][nm]
        start = lead - rng.randrange(0, min(lead, genome["pattern"] - 1) + 1)
        L1, L2 = rng.choice(lengths), rng.choice(lengths)
        flen = rng.randrange(max(L1, L2) + 40, len(text) - start - 8)
        frag = text[start:start + flen]
        a = si.convert(rng, frag[:L1], False, rate=1.0)
        k = len(s1) % 3
        a = put(a, (L1 - 1,)) if k == 1 else put(a, (L1 - 2,)) if k == 2 else a
        s1.append(a)
        s2.append(si.substitute(rng, si.convert(rng, refio.revcomp(frag)[:L2], True), rng.choice([0, 1])))
    return s1, s2
