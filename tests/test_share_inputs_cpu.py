"""The inputs of tests/test_gpu_verify_share_edges.py are decisive (tests/share_inputs.py): on both ends genomes, for
seed patterns 3 and 5, the oracle's record of every unsubstituted family read at a seed shift s > 0 has fewer `times`
than at s = 0 and fewer than the read's exact occurrences in the concatenated strand genomes -- so a verifier that
applies another read's shift to the sequence-bounds test, or none, writes another record.  Host builder and oracle only."""
import os

import pytest

import refio
import share_inputs as si


@pytest.mark.parametrize("fillers", [0, 700])
@pytest.mark.parametrize("pattern", [3, 5])
def test_the_oracle_records_depend_on_the_per_read_bounds_test(scratch, pattern, fillers):
    genome = si.ends_genome(pattern, fillers=fillers)
    assert len(genome["seqs"]) == 434 + fillers and (len(genome["seqs"]) > 1023) == (fillers > 0)
    refio.set_pattern(pattern)
    try:
        fa = os.path.join(scratch, "ends_cpu_%d_%d.fa" % (pattern, fillers))
        si.write_fasta(genome["seqs"], fa)
        path = os.path.join(scratch, "ends_cpu_%d_%d.dbindex" % (pattern, fillers))
        rc = refio.harness().walt_makedb(fa.encode(), path.encode(), 4)
        assert rc == 0, refio.harness().walt_last_error()
        db = refio.DbIndex(path, strands=(0, 1))
        for sfx in refio.STRAND_SUFFIX:  # (64 MB of bucket counters a strand: the arrays are loaded)
            os.remove(path + sfx)
        assert db.n_chrom == len(genome["seqs"])
        for lengths in si.ENDS_LENGTHS[pattern]:
            reads, meta = si.ends_pool(genome, lengths)
            assert len(reads) < 3500
            want, _ = refio.oracle_se(db, reads, ag=False, max_mm=6, b=5000, threads=4)
            si.assert_decisive(db, reads, meta, want, what="pattern %d, %d fillers, lengths %s" % (pattern, fillers, lengths))
            plain = meta["plain"] & (meta["family"] == 0) & (meta["length"] == lengths[0])
            print("pattern %d, %d fillers, lengths %s: times of family 0 at shifts 0 .. : %s" % (
                pattern, fillers, lengths, [int(want["times"][(plain & (meta["shift"] == s))][0]) for s in range(pattern)]))
    finally:
        refio.set_pattern(3)
