"""The inputs of tests/test_gpu_verify_lds.py are decisive (tests/lds_inputs.py): on the ends genome of seed pattern 3,
in every batch, the reads of a (family, lead, length) that has two or more of them do not all have one `mismatch` in the
oracle's records -- a grouped verifier that evaluates a read with another read's operands writes another record.  Host
builder and oracle only."""
import os

import numpy as np
import pytest

import align_inputs as ai
import lds_inputs as li
import refio
import share_inputs as si


@pytest.fixture(scope="module")
def ends_db(scratch):
    genome = si.ends_genome(3)
    fa = os.path.join(scratch, "lds_cpu.fa")
    si.write_fasta(genome["seqs"], fa)
    path = os.path.join(scratch, "lds_cpu.dbindex")
    rc = refio.harness().walt_makedb(fa.encode(), path.encode(), 4)
    assert rc == 0, refio.harness().walt_last_error()
    db = refio.DbIndex(path)
    for sfx in refio.STRAND_SUFFIX:
        os.remove(path + sfx)
    return genome, db


@pytest.mark.parametrize("words", sorted(li.LENGTHS))
def test_no_group_of_reads_has_one_mismatch_count(ends_db, words):
    genome, db = ends_db
    reads, _, meta = ai.pool(genome, li.LENGTHS[words])
    want, _ = refio.oracle_se(db, reads, ag=False, max_mm=6, b=5000, threads=4)
    for case, (families, w) in sorted(li.CASES.items()):
        if w != words:
            continue
        sel = li.select(meta, families)
        li.assert_decisive(want, meta, sel, families, what=case)
        fam = meta["family"][sel] >= 0
        print("%s: %d reads, %d of the families, mismatches %s" % (case, sel.size, int(fam.sum()),
                                                                   np.bincount(want["mismatch"][sel][fam]).tolist()))
