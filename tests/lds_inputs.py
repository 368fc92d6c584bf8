"""Batches for tests/test_gpu_verify_lds.py, cut out of the pools of tests/align_inputs.py on the ends genome of
tests/share_inputs.py -- pure Python, no device; tests/test_lds_inputs_cpu.py proves on the host that they are decisive.

k_se_verify_shared keeps the aligned operands of a unit's reads in a per-wavefront LDS area that is rewritten at every
unit border.  What can go wrong there is a read evaluated with ANOTHER read's operands: those of the unit before (a
stale area), or those of its neighbour in the unit (a wrong record).  So a batch holds, of every (family, lead, length)
of the chosen families, 1, 2, 3, 4, 5 or 9 reads in turn -- the cut makes units of four, three, two and one of them, a unit
of one behind a unit of four among them -- taken from the pool in the order of their kinds: the unsubstituted read first,
then the one with its first base substituted, its last, its last but one, ...  A group of two or more reads then never
has one `mismatch` for all its reads, and a read that is given a neighbour's operands writes another record.  The
background reads of the pool come along."""
import numpy as np

import align_inputs as ai

LENGTHS = {"nw7": ai.LENGTHS[0], "nw8": ai.LENGTHS[2]}  # (100, 109, 110): the 7-word instance; (113, 126, 127, 128): 8 words
COUNTS = (1, 2, 3, 4, 5, 9)
# family 0: 20 copies per strand, one 64-record step per unit -- every step a border; family 2: 130 copies, three steps
CASES = {"borders-nw7": ((0,), "nw7"), "borders-nw8": ((0,), "nw8"), "steps-nw7": ((0, 2), "nw7"), "steps-nw8": ((0, 2), "nw8")}


def select(meta, families):
    """-> the pool's indices of the batch, ascending (the pool is shuffled: leads, lengths and kinds mix in a unit)"""
    take, n = [], 0
    leads = sorted(set(int(v) for v in meta["lead"][meta["family"] >= 0]))
    lengths = sorted(set(int(v) for v in meta["length"][meta["family"] >= 0]))
    for f in families:
        for s in leads:
            for L in lengths:
                mine = np.flatnonzero((meta["family"] == f) & (meta["lead"] == s) & (meta["length"] == L))
                assert mine.size == ai.COPIES
                mine = mine[np.argsort(meta["kind"][mine], kind="stable")]
                take += mine[:COUNTS[n % len(COUNTS)]].tolist()
                n += 1
    take += np.flatnonzero(meta["family"] < 0).tolist()
    return np.array(sorted(take))


def assert_decisive(want, meta, sel, families, what=""):
    """`want`: the oracle's records of the whole pool.  Every family read of the batch maps; every (family, lead, length)
    with two or more reads in the batch has reads of different `mismatch`; every count of COUNTS occurs; the leads 0, 1
    and 2 all occur."""
    m = meta[sel]
    w = want[sel]
    fam = m["family"] >= 0
    assert sorted(set(m["family"][fam].tolist())) == sorted(families)
    assert (w["times"][fam] > 0).all(), "%s: family reads that do not map" % what
    counts = set()
    for key in sorted(set(zip(m["family"][fam].tolist(), m["lead"][fam].tolist(), m["length"][fam].tolist()))):
        g = fam & (m["family"] == key[0]) & (m["lead"] == key[1]) & (m["length"] == key[2])
        counts.add(int(g.sum()))
        if g.sum() >= 2:
            assert len(set(w["mismatch"][g].tolist())) >= 2, "%s %s: one mismatch count %s for all %d reads" % (
                what, key, w["mismatch"][g][0], g.sum())
    assert counts == set(COUNTS), "%s: reads per (family, lead, length) %s" % (what, sorted(counts))
    assert sorted(set(m["lead"][fam].tolist())) == [0, 1, 2]
