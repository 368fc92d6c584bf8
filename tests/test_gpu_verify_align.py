"""The dense verifiers with the read aligned to the record grid once per unit / per item (core.h align_read,
count_mismatch_aligned; map_se.hip k_se_verify_shared, map_items.h item_stream under k_se_verify and k_pe_verify)
against the oracle, where the alignment can go wrong: the edges of the record's words and the word behind them.

Genome: the ends genome of tests/share_inputs.py (170 kb in 434 sequences; families of 20, 66 and 130 copies per strand: one
64-record step, one full step plus two candidates, three steps).  Reads (tests/align_inputs.py): nine per (family,
lead, length) -- full units of four, a unit of one, the seed shifts mixed in a unit -- of 100, 109 and 110 bases (the
7-word instance on dense records), 111 and 112 (7 words, the gather route: longer than a 7-word record holds), 113, 126,
127 and 128 (8 words; at seed shift 0 the bases 127 and 128 lie in the ninth record word), with substitutions at the
read's first, last and last-but-one base.  The oracle says on the CPU that for every (length, lead) some read's record
changes when its last base is ignored.  Schedules: the default, se_verify_share = 0 (k_se_verify: item_stream) and
se_pipe = 0.  And pairs on the same genome through the staged paired-end path (k_pe_verify: item_stream)."""
import os

import numpy as np
import pytest

import align_inputs as ai
import refio
import share_inputs as si
from test_gpu_verify_share import device_run
from test_harness_cpu import assert_best_equal

pytestmark = pytest.mark.gpu

SCHEDULES = [{}, {"se_verify_share": 0}, {"se_pipe": 0}]
NAMES = ("se_verify_share", "se_pipe")


@pytest.fixture(scope="module")
def wa():
    import walt_amd
    assert walt_amd.device_count() >= 1, "no HIP device: the walt_amd hot path has no CPU fallback"
    return walt_amd


@pytest.fixture(scope="module")
def world(wa, scratch):
    genome = si.ends_genome(3)
    fa = os.path.join(scratch, "align.fa")
    si.write_fasta(genome["seqs"], fa)
    path = os.path.join(scratch, "align.dbindex")
    wa.makedb(fa, path, threads=8)
    db = refio.DbIndex(path)
    idx = wa.Index.open(path, device=0)
    yield genome, db, idx
    idx.close()
    for sfx in refio.STRAND_SUFFIX:
        if os.path.exists(path + sfx):
            os.remove(path + sfx)


@pytest.mark.parametrize("lengths", ai.LENGTHS, ids=["nw7", "gather", "nw8"])
def test_records_equal_the_oracle_at_the_word_edges(wa, world, index_options, lengths):
    genome, db, idx = world
    reads, restored, meta = ai.pool(genome, lengths)
    want, _ = refio.oracle_se(db, reads, ag=False, max_mm=6, b=5000, threads=8)
    want_restored, _ = refio.oracle_se(db, restored, ag=False, max_mm=6, b=5000, threads=8)
    ai.assert_decisive(want, want_restored, meta, what="lengths %s" % (lengths,))
    defaults = {name: idx.get_option(name) for name in NAMES}
    assert defaults == {"se_verify_share": 1, "se_pipe": 1}
    first = None
    for sched in SCHEDULES:
        index_options(idx, **{name: sched.get(name, defaults[name]) for name in NAMES})
        raw, stats, rode, recs = device_run(wa, idx, reads, 6)
        got = np.frombuffer(raw[:16 * len(reads)], dtype=wa.best_match_dtype)
        assert_best_equal(got, want, "lengths %s %s" % (lengths, sched))
        first = (raw, stats) if first is None else first
        assert (raw, stats) == first, "lengths %s %s: bytes or statistics differ from the default schedule's" % (lengths, sched)
        if sched.get("se_verify_share", 1) == 0:
            assert rode == 0
        elif max(lengths) != 112:  # (the reads of 111 and 112 bases are no dense items: nothing to group)
            assert rode > 0 and 0 < recs[1] < recs[0], "lengths %s %s: no item rode along (%d), records %s" % (lengths, sched, rode, recs)


@pytest.mark.parametrize("lengths", [ai.LENGTHS[0], ai.LENGTHS[2]], ids=["nw7", "nw8"])
def test_pairs_equal_the_oracle(wa, world, lengths):
    genome, db, idx = world
    s1, s2 = ai.pairs(genome, lengths)
    want, _, _ = refio.oracle_pe(db, s1, s2, max_mm=6, b=5000, top_k=50, frag_range=1000, threads=8)
    assert (want["best_times"] > 0).mean() > 0.5 and (want["m1"]["mismatch"][1::3] >= 1).all()
    res, _ = idx.map_pe_batch(*wa.pack_reads(s1), *wa.pack_reads(s2), max_mismatches=6, b=5000, top_k=50, frag_range=1000)
    for f in ("best_times", "frag_len", "best_i", "best_j", "pair_mm"):
        assert np.array_equal(res[f], want[f]), (lengths, f)
    assert_best_equal(res["m1"], want["m1"], "pair m1 %s" % (lengths,))
    assert_best_equal(res["m2"], want["m2"], "pair m2 %s" % (lengths,))
