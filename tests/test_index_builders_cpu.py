"""The host index builder (walt_makedb, walt_amd/csrc/host_index.cpp) against a plain numpy restatement of the
reference's BuildIndex (tests/indexref.py) and, where oracle/_ref/makedb exists, the real binary's files, on genomes
that reach what the golden genome and the random genomes of the other tests do not:
  erase    a bucket of exactly 500,000 positions (erased) beside one of exactly 499,999 (kept), on every strand;
  edges    sequences of 1, 20, 35, 36, 37, 38, 51 and 100 bases, a sequence start at 15 mod 16, a total length that
           is no multiple of 16, a last sequence of 37 bases;
  ends     one bucket with entries whose room runs out at every care character, exact duplicates (tie runs) and
           more than 2,048 sequences;
  tiefree  random, no two entries with equal keys: compared byte for byte.
Every comparison is exact, or exact up to the order inside runs of fully equal keys; the runs come from the
restatement (indexref.same_up_to_ties), never from the builder under test.

Measured where this was written: the restatement of `erase` (four strands of 1.1 Mbp) takes 4.4 s and the solving of
its run lengths 1.8 s; the host builder needs 1.6 s for that genome (4 threads) and the real makedb 6.1 s."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import indexref
import refio


class Cases:
    """genome, restatement, FASTA and host-built files per (genome name, seed pattern), each made once"""

    def __init__(self, scratch):
        self.scratch = scratch
        self.made = {}

    def get(self, name, pattern=3):
        key = (name, pattern)
        if key not in self.made:
            seqs = indexref.RECIPES[name](pattern)
            ref = indexref.build(seqs, pattern)
            indexref.assert_recipe(name, ref)  # the input's conditions, before any builder is consulted
            fa = os.path.join(self.scratch, "ib_%s_%d.fa" % (name, pattern))
            indexref.write_fasta(fa, seqs)
            out = os.path.join(self.scratch, "ib_%s_%d.dbindex" % (name, pattern))
            refio.set_pattern(pattern)
            try:
                rc = refio.harness().walt_makedb(fa.encode(), out.encode(), 4)
                assert rc == 0, refio.harness().walt_last_error()
            finally:
                refio.set_pattern(3)
            self.made[key] = (seqs, ref, fa, out)
        return self.made[key]


@pytest.fixture(scope="module")
def cases(scratch):
    return Cases(scratch)


def assert_files_equal_restatement(path, ref, exact_index, what):
    db = refio.DbIndex(path)
    assert db.names == ref.names, what
    assert np.array_equal(db.lengths, ref.lengths), what
    assert db.genome_len == ref.genome_len and db.max_index_size == ref.max_index_size, what
    for s in range(4):
        r = ref.strand[s]
        with open(path + refio.STRAND_SUFFIX[s], "rb") as f:
            assert f.read(1) == (b"-" if s & 1 else b"+"), "%s strand %d sign" % (what, s)
        assert np.array_equal(db.genome[s], r.genome), "%s strand %d genome" % (what, s)
        assert np.array_equal(db.counter[s], r.counter), "%s strand %d counter" % (what, s)
        assert db.index[s].size == r.index_size, "%s strand %d index size" % (what, s)
        assert indexref.same_up_to_ties(db.index[s], r), "%s strand %d index order" % (what, s)
        if exact_index:
            assert np.array_equal(db.index[s], r.index), "%s strand %d index" % (what, s)
    return db


@pytest.mark.parametrize("name", ["erase", "edges", "ends", "tiefree"])
def test_host_builder_equals_restatement(cases, name):
    _, ref, _, out = cases.get(name)
    assert_files_equal_restatement(out, ref, name == "tiefree", "host builder, " + name)


def _md5(path):
    h = hashlib.md5()
    with open(path, "rb") as f:
        for blk in iter(lambda: f.read(1 << 22), b""):
            h.update(blk)
    return h.hexdigest()


@pytest.mark.parametrize("name", ["erase", "edges", "tiefree"])
def test_reference_makedb_equals_restatement(cases, scratch, name):
    """The real binary's files against the restatement (and so, with the test above, against the host builder); on
    the tie-free genome the host builder's strand files are also md5-identical to the real binary's."""
    if not os.path.exists(refio.ref_makedb()):
        pytest.skip("reference makedb not built (oracle/_ref)")
    _, ref, fa, host = cases.get(name)
    out = os.path.join(scratch, "ib_ref_%s.dbindex" % name)
    subprocess.run([refio.ref_makedb(), "-c", fa, "-o", out], check=True, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL)
    assert_files_equal_restatement(out, ref, name == "tiefree", "reference makedb, " + name)
    if name == "tiefree":
        for sfx in ("",) + refio.STRAND_SUFFIX:
            assert _md5(host + sfx) == _md5(out + sfx), sfx


@pytest.mark.parametrize("pattern", [5, 7])
@pytest.mark.parametrize("name", ["edges", "ends"])
def test_host_builder_equals_restatement_patterns(cases, name, pattern):
    _, ref, _, out = cases.get(name, pattern)
    assert_files_equal_restatement(out, ref, False, "host builder, pattern %d, %s" % (pattern, name))


def test_host_builder_all_short_genome(scratch):
    """Every sequence below MINIMALSEEDLEN: nothing is hashed, counter[] is all zero and index[] is empty
    (CountBucketSize skips such sequences, reference.cpp:200-201)."""
    rs = np.random.RandomState(24)
    seqs = [("t%d" % i, indexref.random_sequence(rs, n)) for i, n in enumerate((35, 1, 20, 35, 7))]
    ref = indexref.build(seqs)
    assert ref.max_index_size == 0 and all(not r.counter.any() and r.index.size == 0 for r in ref.strand)
    fa, out = os.path.join(scratch, "ib_short.fa"), os.path.join(scratch, "ib_short.dbindex")
    indexref.write_fasta(fa, seqs)
    assert refio.harness().walt_makedb(fa.encode(), out.encode(), 2) == 0
    assert_files_equal_restatement(out, ref, True, "host builder, all-short genome")
    if os.path.exists(refio.ref_makedb()):
        real = os.path.join(scratch, "ib_short_ref.dbindex")
        subprocess.run([refio.ref_makedb(), "-c", fa, "-o", real], check=True, stdout=subprocess.DEVNULL,
                       stderr=subprocess.DEVNULL)
        for sfx in ("",) + refio.STRAND_SUFFIX:
            assert _md5(out + sfx) == _md5(real + sfx), sfx


def test_same_up_to_ties_is_strict():
    """The one exception the comparisons allow, pinned: a permutation inside a tie run passes; an entry moved out of
    its run, two runs' entries exchanged, or any change outside the runs does not."""
    seqs = indexref.genome_ends()
    r = indexref.build(seqs, strands=(0,)).strand[0]
    assert indexref.same_up_to_ties(r.index, r) and indexref.ascending_in_tie_runs(r.index, r)
    inside = np.nonzero(r.ties[:-1] & (r.run_id[1:] == r.run_id[:-1]))[0]
    i = int(inside[0])
    swapped = r.index.copy()
    swapped[[i, i + 1]] = swapped[[i + 1, i]]
    assert indexref.same_up_to_ties(swapped, r) and not indexref.ascending_in_tie_runs(swapped, r)
    across = np.nonzero(r.run_id[1:] != r.run_id[:-1])[0]
    for j in (int(across[0]), int(across[across.size // 2])):
        bad = r.index.copy()
        bad[[j, j + 1]] = bad[[j + 1, j]]
        assert not indexref.same_up_to_ties(bad, r), j
    touching = np.nonzero(r.ties[:-1] & r.ties[1:] & (r.run_id[1:] != r.run_id[:-1]))[0]
    assert touching.size > 0  # two tie runs next to each other: the mask alone would let their entries cross
    assert not indexref.same_up_to_ties(r.index[:-1], r)
