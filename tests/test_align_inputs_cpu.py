"""The inputs of tests/test_gpu_verify_align.py are decisive (tests/align_inputs.py): on the ends genome of seed pattern
3, for every batch of lengths, every length and every lead, the oracle's record of some read changes when the read's
last base is ignored -- so a dense verifier that leaves the word behind the record's NW out where the read reaches it,
or compares it where the read does not, writes another record.  Host builder and oracle only."""
import os

import numpy as np
import pytest

import align_inputs as ai
import refio
import share_inputs as si


@pytest.fixture(scope="module")
def ends_db(scratch):
    genome = si.ends_genome(3)
    fa = os.path.join(scratch, "align_cpu.fa")
    si.write_fasta(genome["seqs"], fa)
    path = os.path.join(scratch, "align_cpu.dbindex")
    rc = refio.harness().walt_makedb(fa.encode(), path.encode(), 4)
    assert rc == 0, refio.harness().walt_last_error()
    db = refio.DbIndex(path)  # (the second mates of the pairs map on the G->A strands)
    for sfx in refio.STRAND_SUFFIX:
        os.remove(path + sfx)
    return genome, db


@pytest.mark.parametrize("lengths", ai.LENGTHS, ids=["nw7", "gather", "nw8"])
def test_records_depend_on_the_last_base(ends_db, lengths):
    genome, db = ends_db
    reads, restored, meta = ai.pool(genome, lengths)
    assert len(reads) == 3 * 3 * len(lengths) * ai.COPIES + ai.N_BACKGROUND and [len(r) for r in reads] == meta["length"].tolist()
    want, _ = refio.oracle_se(db, reads, ag=False, max_mm=6, b=5000, threads=4)
    want_restored, _ = refio.oracle_se(db, restored, ag=False, max_mm=6, b=5000, threads=4)
    ai.assert_decisive(want, want_restored, meta, what="lengths %s" % (lengths,))
    fam = meta["family"] >= 0
    print("lengths %s: mismatches of the family reads %s, times %s" % (lengths, np.bincount(want["mismatch"][fam]).tolist(),
                                                                       sorted(set(want["times"][fam].tolist()))[:12]))


def test_pairs_map_in_their_families(ends_db):
    genome, db = ends_db
    for lengths in (ai.LENGTHS[0], ai.LENGTHS[2]):
        s1, s2 = ai.pairs(genome, lengths)
        want, _, _ = refio.oracle_pe(db, s1, s2, max_mm=6, b=5000, top_k=50, frag_range=1000, threads=4)
        # (a first mate has up to 130 equally good places and the 50 best are kept: its own copy is among them for most pairs)
        assert (want["best_times"] > 0).mean() > 0.5, "lengths %s: %.2f of the pairs map" % (lengths, (want["best_times"] > 0).mean())
        assert (want["m1"]["mismatch"][1::3] >= 1).all()  # (the substituted last base of every third first mate counts)
