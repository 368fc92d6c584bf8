"""The grouped dense verifier (map_se.hip k_se_verify_shared) where tests/test_gpu_verify_share.py does not reach:
  * repeat copies within kPat - 1 bases of the START of their sequence on either strand, met by reads of every seed
    shift and of several lengths in one unit -- the only place where the per-read sequence-bounds test rejects a
    candidate of a dense record (tests/share_inputs.py; tests/test_share_inputs_cpu.py proves on the host that the
    oracle's records there depend on the read's own shift) -- with 434 sequences (the LDS table of sequence starts)
    and with 1,134 (walt::chrom_bounds), and the edge bit set in front of both;
  * the 8-word instance (reads of 113 to 128 bases: win2, eight read words, masks from header quads 4 and 5), alone
    and with 100-base reads in the same units, on the ends genomes and on a ladder of regions up to 1,025 candidates;
  * -b below a family's size; the G->A strands (strand_base = 2); map_se_rpbat_batch (both passes over one workspace);
  * seed pattern 5 (grouped at 7 words with five rounds a chunk, not at 8) and 7 (never grouped).
Every case: the records equal the oracle's, the raw record bytes and the statistics equal those of se_verify_share = 0,
and the control words say that items rode along (or that none did, where the route is not grouped)."""
import os

import numpy as np
import pytest

import refio
import share_inputs as si
from test_gpu_rpbat import assert_records, rpbat_rule
from test_gpu_verify_share import device_run
from test_harness_cpu import assert_best_equal

pytestmark = pytest.mark.gpu

SCHEDULES = [{}, {"se_share_cap": 7}, {"grid": 1}, {"se_heavy_chunk": 320}]
NAMES = ("se_share_cap", "grid", "se_heavy_chunk")
NW7, NW8, MIXED = si.ENDS_LENGTHS[3]


@pytest.fixture(scope="module")
def wa():
    import walt_amd
    assert walt_amd.device_count() >= 1, "no HIP device: the walt_amd hot path has no CPU fallback"
    return walt_amd


class World:
    """a genome indexed once, opened once; the oracle's records once per batch"""

    def __init__(self, wa, scratch, name, seqs, all_strands=False):
        self.wa = wa
        fa = os.path.join(scratch, name + ".fa")
        si.write_fasta(seqs, fa)
        self.path = os.path.join(scratch, name + ".dbindex")
        wa.makedb(fa, self.path, threads=8)
        self.db = refio.DbIndex(self.path, strands=(0, 1, 2, 3) if all_strands else (0, 1))
        self.idx = wa.Index.open(self.path, device=0, strands=wa.STRANDS_ALL if all_strands else wa.STRANDS_CT)
        self.cache = {}

    def oracle(self, key, reads, ag=False, b=5000):
        k = (key, ag, b)
        if k not in self.cache:
            self.cache[k] = refio.oracle_se(self.db, reads, ag=ag, max_mm=6, b=b, threads=8)[0]
        return self.cache[k]

    def close(self):
        self.idx.close()
        for sfx in refio.STRAND_SUFFIX:
            if os.path.exists(self.path + sfx):
                os.remove(self.path + sfx)


@pytest.fixture(scope="module")
def ends(wa, scratch):
    """the two ends genomes of seed pattern 3: fillers -> (genome, World)"""
    worlds = {}
    for fillers in (0, 700):
        genome = si.ends_genome(3, fillers=fillers)
        worlds[fillers] = (genome, World(wa, scratch, "ends_%d" % fillers, genome["seqs"], all_strands=fillers == 0))
    assert worlds[0][1].db.n_chrom == 434 <= 1023 < worlds[700][1].db.n_chrom
    yield worlds
    for _, w in worlds.values():
        w.close()


@pytest.fixture(scope="module")
def ladder(wa, scratch):
    seqs, copies = si.long_ladder()
    w = World(wa, scratch, "long_ladder", seqs)
    reads, family = si.ladder_pool(seqs, copies)
    want = w.oracle("pool", reads)
    yield w, reads, family, want
    w.close()


def records_of(wa, raw, n):
    return np.frombuffer(raw[:16 * n], dtype=wa.best_match_dtype)


def check(wa, idx, index_options, reads, want, expect, what, schedules=({},), twice=False, **call):
    """Under every schedule: se_verify_share = 0 gives the oracle's records; se_verify_share = 1 gives the same bytes
    and statistics -- twice: also on the slots and cursors its first call left -- and the expected observation:
    "rides": items rode along and the units' records are fewer than the items' (under se_share_cap = 7: a bound, see
    below); "alone": nothing rode along.
    want: the oracle's records, or (records, conversions) of a random-PBAT call.  -> items that rode along"""
    n = len(reads)
    defaults = {name: idx.get_option(name) for name in NAMES}
    first, rode = None, 0
    for sched in schedules:
        index_options(idx, **{name: sched.get(name, defaults[name]) for name in NAMES})
        index_options(idx, se_verify_share=0)
        rec0, st0, rode0, _ = device_run(wa, idx, reads, 6, **call)
        assert rode0 == 0
        first = (rec0, st0) if first is None else first
        assert (rec0, st0) == first, "%s %s: the ungrouped verifier's records or statistics differ from the first schedule's" % (what, sched)
        index_options(idx, se_verify_share=1)
        for again in range(2 if twice else 1):
            tag = "%s %s call %d" % (what, sched, again)
            rec1, st1, rode, recs = device_run(wa, idx, reads, 6, **call)
            print("%s: expected %s, %d items rode along, records of items / of units %s" % (tag, expect, rode, recs))
            for raw, share in ((rec0, 0), (rec1, 1)):
                if call.get("rpbat"):
                    assert_records(records_of(wa, raw, n), np.frombuffer(raw[16 * n:], dtype=np.uint8), want[0], want[1], "%s share=%d" % (tag, share))
                else:
                    assert_best_equal(records_of(wa, raw, n), want, "%s share=%d" % (tag, share))
            assert rec1 == rec0 and st1 == st0, "%s: bytes or statistics differ from se_verify_share = 0: %s, %s" % (tag, st1, st0)
            cap = sched.get("se_share_cap", 0)
            if expect == "rides" and cap > 1:
                # Only the first `cap` items of a (chunk, round) are grouped, in the order the stage kernel's wavefronts
                # appended them: whether two of those seven name one region differs from call to call (measured on
                # these batches: 0 .. 5 items rode along).  What is certain is the bound, and that every item behind
                # the cap is verified as a unit of one with the same bytes.
                assert rode <= (cap - 1) * 8 * call.get("pat", 3) and 0 < recs[1] <= recs[0], "%s: %d items rode along, records %s" % (tag, rode, recs)
            elif expect == "rides":
                assert rode > 0 and 0 < recs[1] < recs[0], "%s: no item rode along (%d), records of items / of units %s" % (tag, rode, recs)
            else:
                assert expect == "alone" and rode == 0, "%s: %d items rode along on a route that is not grouped" % (tag, rode)
    return rode


@pytest.mark.parametrize("lengths", [NW7, NW8, MIXED], ids=["nw7", "nw8", "mixed"])
@pytest.mark.parametrize("fillers", [0, 700])
def test_copies_at_sequence_starts(wa, ends, index_options, fillers, lengths):
    genome, w = ends[fillers]
    reads, meta = si.ends_pool(genome, lengths)
    want = w.oracle(lengths, reads)
    si.assert_decisive(w.db, reads, meta, want, what="%d fillers, lengths %s" % (fillers, lengths))
    assert len(reads) < 3500 and len(set(int(s) for s in meta["shift"][meta["family"] >= 0])) == 3
    check(wa, w.idx, index_options, reads, want, "rides", "ends genome, %d fillers, lengths %s" % (fillers, lengths), schedules=SCHEDULES, twice=True)


@pytest.mark.parametrize("lengths", [NW7, NW8], ids=["nw7", "nw8"])
def test_b_below_a_family(wa, ends, index_options, lengths):
    """-b 100: the family of 130 copies per strand exceeds it, those of 20 and 66 do not (and still ride along)"""
    genome, w = ends[0]
    reads, meta = si.ends_pool(genome, lengths)
    want = w.oracle(lengths, reads, b=100)
    full = w.oracle(lengths, reads)
    big = (meta["family"] == 2) & meta["plain"]
    assert (full["times"][big] > 100).any() and not np.array_equal(want["times"][big], full["times"][big])  # (-b decides records here)
    check(wa, w.idx, index_options, reads, want, "rides", "-b 100, lengths %s" % (lengths,), b=100)


@pytest.mark.parametrize("m", [2, 5, 9, 130])
def test_long_ladder(wa, ladder, index_options, m):
    w, pool, family, want_all = ladder
    sel = si.ladder_batch(family, m)
    reads, want = [pool[i] for i in sel], want_all[sel]
    assert 2000 < len(reads) < 3500 and (want["times"] > 0).mean() > 0.8 and max(len(r) for r in reads) == 128
    check(wa, w.idx, index_options, reads, want, "rides", "long ladder m=%d" % m)
    index_options(w.idx, se_share_cap=1)  # every item a unit of its own: nothing rides along, the same records
    check(wa, w.idx, index_options, reads, want, "alone", "long ladder m=%d, se_share_cap=1" % m)


@pytest.mark.parametrize("lengths", [NW7, NW8], ids=["nw7", "nw8"])
def test_other_entry_points(wa, ends, index_options, lengths):
    genome, w = ends[0]
    ct, ct_meta = si.ends_pool(genome, lengths)
    ga, ga_meta = si.ends_pool(genome, lengths, ag=True)
    # the G->A strands: strand_base = 2
    want_ga = w.oracle((lengths, "ga"), ga, ag=True)
    si.assert_decisive(w.db, ga, ga_meta, want_ga, ag=True, what="G->A, lengths %s" % (lengths,))
    check(wa, w.idx, index_options, ga, want_ga, "rides", "ag_wildcard, lengths %s" % (lengths,), ag=True)
    # random PBAT: both passes over one workspace, the share area cleared between them; both conversions of every read
    both = ct + ga
    c, g = w.oracle((lengths, "both"), both), w.oracle((lengths, "both"), both, ag=True)
    rec, conv, rule = rpbat_rule(c, g)
    assert (rule == 2).sum() > 100 and (rule == 3).sum() > 100  # either conversion decides reads of this batch
    check(wa, w.idx, index_options, both, (rec, conv), "rides", "random PBAT, lengths %s" % (lengths,), rpbat=True)
    host, host_conv, _ = w.idx.map_se_rpbat_batch(*wa.pack_reads(both))
    assert_records(host, host_conv, rec, conv, "random PBAT, host form")
    # and the plain call on what the random-PBAT call left
    check(wa, w.idx, index_options, ct, w.oracle(lengths, ct), "rides", "C->T after random PBAT, lengths %s" % (lengths,))


@pytest.fixture  # per test: the module's other tests run on pattern 3 (and in front of index_options, which it outlives)
def pattern_ends(wa, scratch):
    """pattern_ends(p) -> (genome, World): the ends genome of seed pattern p, indexed and opened by that pattern's library"""
    made = []

    def make(p):
        refio.set_pattern(p)
        wa.set_pattern(p)
        genome = si.ends_genome(p)
        assert sorted(set(genome["leads"].values())) == sorted(si.leads_of(p))
        made.append(World(wa, scratch, "ends_sp%d" % p, genome["seqs"]))
        return genome, made[-1]

    try:
        yield make
        for w in made:
            w.close()
    finally:
        refio.set_pattern(3)
        wa.set_pattern(3)


def test_pattern_5_groups_at_seven_words_only(wa, pattern_ends, index_options):
    """libwalt_amd_sp5.so: share_nw<7>() holds (five rounds a chunk, shifts 0 .. 4); the 8-word instance has seeds beyond
    the key characters and keeps the ungrouped verifier"""
    genome, w = pattern_ends(5)
    for lengths, expect in zip(si.ENDS_LENGTHS[5], ("rides", "alone")):
        reads, meta = si.ends_pool(genome, lengths)
        want = w.oracle(lengths, reads)
        si.assert_decisive(w.db, reads, meta, want, what="pattern 5, lengths %s" % (lengths,))
        assert int(meta["shift"].max()) == 4
        check(wa, w.idx, index_options, reads, want, expect, "pattern 5, lengths %s" % (lengths,), twice=True, pat=5)


def test_pattern_7_is_not_grouped(wa, pattern_ends, index_options):
    """libwalt_amd_sp7.so: every instance has seeds beyond the key characters (share_nw is false): leads and shifts 0 .. 6"""
    genome, w = pattern_ends(7)
    (lengths,) = si.ENDS_LENGTHS[7]
    reads, meta = si.ends_pool(genome, lengths)
    want = w.oracle(lengths, reads)
    si.assert_decisive(w.db, reads, meta, want, what="pattern 7")
    assert int(meta["shift"].max()) == 6
    check(wa, w.idx, index_options, reads, want, "alone", "pattern 7", pat=7)
