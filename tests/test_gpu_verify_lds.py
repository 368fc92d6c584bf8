"""The grouped dense verifier with a unit's aligned operands in LDS (map_se.hip k_se_verify_shared; core.h operand_slot):
a per-wavefront area, written at every unit border and read back by every step.  Where that can go wrong --

* stale operands across unit borders: reads of the 20-copy family of the ends genome (tests/share_inputs.py), whose units
  are one 64-record step, so that every step is a border; 1, 2, 3, 4, 5 and 9 reads per (lead, length), which the cut
  makes into units of four, three, two and one, a unit of one behind a unit of four among them; on one block (grid = 1:
  four wavefronts walk all units in turn), on one stream (se_pipe = 0) and on the default schedule;
* steps within a unit that read the same operands again: the same with the 130-copy family, three steps, in the batch;
* the operands of the right read: seed shifts 0, 1 and 2 in one unit, and per read one substitution at another place --
  the first, the last, the last-but-one base (tests/align_inputs.py), so that no two reads of a group have one record;
* both instances: reads of 100, 109 and 110 bases (7 words), of 113, 126, 127 and 128 (8 words: the top words are
  operands too);
* an area that nobody has written when the kernel starts: every batch twice on one index, the bytes compared.

Every case: the records equal the oracle's, records and statistics are byte-identical to the run with
se_verify_share = 0, and items rode along, so the grouped verifier ran.  tests/test_lds_inputs_cpu.py proves the
batches decisive on the host; the same assertion is made here on the oracle's records before anything runs."""
import os

import numpy as np
import pytest

import align_inputs as ai
import lds_inputs as li
import refio
import share_inputs as si
from test_gpu_verify_share import device_run
from test_harness_cpu import assert_best_equal

pytestmark = pytest.mark.gpu

SCHEDULES = [{"grid": 1}, {"se_pipe": 0}, {}]
NAMES = ("grid", "se_pipe", "se_verify_share")


@pytest.fixture(scope="module")
def wa():
    import walt_amd
    assert walt_amd.device_count() >= 1, "no HIP device: the walt_amd hot path has no CPU fallback"
    return walt_amd


@pytest.fixture(scope="module")
def world(wa, scratch):
    genome = si.ends_genome(3)
    fa = os.path.join(scratch, "lds.fa")
    si.write_fasta(genome["seqs"], fa)
    path = os.path.join(scratch, "lds.dbindex")
    wa.makedb(fa, path, threads=8)
    db = refio.DbIndex(path)
    idx = wa.Index.open(path, device=0)
    pools = {}
    for words, lengths in li.LENGTHS.items():  # the oracle once per pool, shared by the cases
        reads, _, meta = ai.pool(genome, lengths)
        want, _ = refio.oracle_se(db, reads, ag=False, max_mm=6, b=5000, threads=8)
        pools[words] = (reads, meta, want)
    yield idx, pools
    idx.close()
    for sfx in refio.STRAND_SUFFIX:
        if os.path.exists(path + sfx):
            os.remove(path + sfx)


@pytest.mark.parametrize("case", sorted(li.CASES))
def test_every_read_meets_its_own_operands(wa, world, index_options, case):
    idx, pools = world
    families, words = li.CASES[case]
    pool_reads, meta, pool_want = pools[words]
    sel = li.select(meta, families)
    li.assert_decisive(pool_want, meta, sel, families, what=case)
    reads, want = [pool_reads[i] for i in sel], pool_want[sel]
    defaults = {name: idx.get_option(name) for name in NAMES}
    assert defaults["se_verify_share"] == 1 and defaults["se_pipe"] == 1
    index_options(idx, **dict(defaults, se_verify_share=0))
    plain = device_run(wa, idx, reads, 6)
    assert plain[2] == 0
    assert_best_equal(np.frombuffer(plain[0][:16 * len(reads)], dtype=wa.best_match_dtype), want, "%s ungrouped" % case)
    for sched in SCHEDULES:
        index_options(idx, **dict({name: sched.get(name, defaults[name]) for name in NAMES}, se_verify_share=1))
        for call in range(2):
            raw, stats, rode, recs = device_run(wa, idx, reads, 6)
            what = "%s %s call %d" % (case, sched, call)
            assert_best_equal(np.frombuffer(raw[:16 * len(reads)], dtype=wa.best_match_dtype), want, what)
            assert raw == plain[0] and stats == plain[1], "%s: bytes or statistics differ from se_verify_share = 0" % what
            assert rode > 0 and 0 < recs[1] < recs[0], "%s: no item rode along (%d), records %s" % (what, rode, recs)
