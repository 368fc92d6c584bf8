"""Dense items grouped by region (option se_verify_share; walt_amd/csrc/group_core.h, map_se.hip k_se_share_*,
k_se_verify_shared): the records and statistics of every batch equal the oracle's and those of se_verify_share = 0, under
every schedule the grouping meets.

Genome in the manner of tests/test_gpu_stage_trips.py's ladder (1.9 Mbp, three sequences): each family is N identical
motifs with random spacers, every second copy reverse-complemented, so that a read of the family names a region of
N / 2 candidates per strand.  The motif has 104 bases and the spacer 20: the seed of a 100-base read spans 32 care
characters, 96 bases, and a region is the candidates equal in ALL of them -- with that ladder's 72-base motifs the last
eight characters fall into the random spacers, a region is the read's own copy, and 3,040 reads made two dense items
(measured); with 104 the whole seed lies in the motif at every seed shift.  N = 34 .. 9,998: one 64-record step and its borders (126, 128, 130), one record
past two steps (258), either side of kBigFirst (2,048 / 2,050) and just under -b 5000 per strand (9,998).  A batch
holds m reads of EVERY family -- m = 1, 2, R, R + 1, 2 R + 1 and 130 for the default R = 4 -- over seed shifts 0, 1, 2,
both read strands and 0 .. 3 substitutions, among 2,000 unique background reads; one batch of 150-base reads takes the
route of the longer reads, which is not grouped.  The oracle's records are computed once per pool."""
import os
import random

import numpy as np
import pytest

import refio
from test_gpu_stage_trips import _rand, convert, substitute
from test_harness_cpu import assert_best_equal

pytestmark = pytest.mark.gpu

MOTIF, SPACER = 104, 20
FAMILIES = [34, 126, 128, 130, 258, 2048, 2050, 9998]
R = 4
SHARED = [1, 2, R, R + 1, 2 * R + 1, 130]
N_BACKGROUND = 2000
# (se_heavy_chunk = 384: eight chunks hold every batch here, so the hook applies: two streams, two state slots)
SCHEDULES = [{}, {"se_pipe": 0}, {"se_heavy_chunk": 320}, {"se_heavy_chunk": 384}, {"grid": 1}, {"grid": 3}, {"se_share_cap": 7},
             {"se_share_cap": 100}]
NAMES = ("se_pipe", "se_heavy_chunk", "grid", "se_share_cap", "se_verify_share")


def read_from_copy(rng, seqs, copy, L):
    """a read that meets the copy's motif at seed 0, 1 or 2, from either strand, converted, with 0 .. 3 substitutions"""
    s, pos, fam, rc = copy
    g = seqs[s][1]
    off = rng.choice([0, 1, 2])
    if rc:  # the motif's first base is the unit's last: the read is taken from the other strand
        end = pos + MOTIF + SPACER + off
        frag = refio.revcomp(g[end - L:end])
    else:
        frag = g[pos - off:pos - off + L]
    assert len(frag) == L
    if rng.random() < 0.15:
        frag = refio.revcomp(frag)
    return substitute(rng, convert(rng, frag, False), rng.choice([0, 1, 1, 2, 2, 3]))


@pytest.fixture(scope="module")
def wa():
    import walt_amd
    assert walt_amd.device_count() >= 1, "no HIP device: the walt_amd hot path has no CPU fallback"
    return walt_amd


@pytest.fixture(scope="module")
def world(wa, scratch):
    rng = random.Random(4711)
    units = []
    for N in FAMILIES:
        motif = _rand(rng, MOTIF)
        units += [(N, motif + _rand(rng, SPACER), k % 2 == 1) for k in range(N)]
    rng.shuffle(units)
    seqs, copies = [], []
    per = (len(units) + 2) // 3
    for s in range(3):
        parts, pos = [_rand(rng, 30000)], 30000
        for fam, text, rc in units[s * per:(s + 1) * per]:
            copies.append((s, pos, fam, rc))
            parts.append(refio.revcomp(text) if rc else text)
            pos += len(text)
        parts.append(_rand(rng, 30000))
        seqs.append(("share%d" % s, "".join(parts)))
    fa = os.path.join(scratch, "share.fa")
    with open(fa, "w") as f:
        for nm, s in seqs:
            f.write(">%s\n%s\n" % (nm, s))
    path = os.path.join(scratch, "share.dbindex")
    wa.makedb(fa, path, threads=8)
    db = refio.DbIndex(path)
    idx = wa.Index.open(path, device=0, strands=wa.STRANDS_CT)
    pools = {}
    for L, max_mm in ((100, 6), (150, 10)):
        reads, family = [], []
        for N in FAMILIES:
            mine = [c for c in copies if c[2] == N]
            # the family's first two reads are MADE for one region: two forward copies, seed shift 0, fully converted, no
            # substitution -- the other 128 are spread over seed shifts, strands and substitutions
            for s_, pos, _, _ in [c for c in mine if not c[3]][:2]:
                reads.append(convert(rng, seqs[s_][1][pos:pos + L], False, rate=1.0))
                family.append(N)
            for _ in range(128):
                reads.append(read_from_copy(rng, seqs, rng.choice(mine), L))
                family.append(N)
        for _ in range(N_BACKGROUND):
            nm, g = seqs[rng.randrange(3)]
            p = rng.choice([rng.randrange(0, 30000 - L), len(g) - 30000 + rng.randrange(0, 30000 - L)])
            frag = g[p:p + L]
            frag = refio.revcomp(frag) if rng.random() < 0.5 else frag
            reads.append(substitute(rng, convert(rng, frag, False), rng.choice([0, 1, 2, 3])))
            family.append(0)
        want, _ = refio.oracle_se(db, reads, ag=False, max_mm=max_mm, b=5000, threads=8)
        pools[L] = {"reads": reads, "family": np.array(family), "want": want, "max_mm": max_mm}
    yield {"idx": idx, "pools": pools}
    idx.close()


def batch_of(pool, m):
    """m reads of every family (the pool's first m of each) and every background read, shuffled the same way every time"""
    fam = pool["family"]
    sel = np.concatenate([np.flatnonzero(fam == N)[:m] for N in FAMILIES] + [np.flatnonzero(fam == 0)])
    return np.random.RandomState(m).permutation(sel)


LAST = {}  # the last device_run's control words


def device_run(wa, idx, reads, max_mm, pat=3, ag=False, b=5000, rpbat=False):
    """one call of the device form -> (records as raw bytes, statistics, control word 7 summed over (chunk, round),
    [records of all items, records of all units] summed).  pat: the seed pattern of the library idx was opened with --
    the staged pass has 8 * pat (chunk, round) pairs (map_se.hip kShareRounds); ag: the G->A strands; rpbat:
    map_se_rpbat_batch_device, the conversion bytes behind the records, the control words those of its second pass"""
    import torch
    dev = torch.device("cuda:0")
    bases, offsets = wa.pack_reads(reads)
    n = offsets.size - 1
    max_len = int((offsets[1:] - offsets[:-1]).max())
    d_bases = torch.from_numpy(bases).to(dev)
    d_off = torch.from_numpy(offsets.astype(np.int64)).to(dev)
    d_out = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    d_conv = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_stats = torch.zeros(4, dtype=torch.int64, device=dev)
    se_ws = wa.lib(pat).walt_se_workspace_bytes(n, max_len)  # (a random-PBAT call lays the same workspace out in front of its second record array)
    ws = wa.lib(pat).walt_se_rpbat_workspace_bytes(n, max_len) if rpbat else se_ws
    d_ws = torch.empty(ws, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    if rpbat:
        idx.map_se_rpbat_batch_device(d_bases.data_ptr(), d_off.data_ptr(), n, max_len, d_out.data_ptr(), d_conv.data_ptr(), d_stats.data_ptr(),
                                      d_ws.data_ptr(), ws, stream=stream, max_mismatches=max_mm, b=b)
    else:
        idx.map_se_batch_device(d_bases.data_ptr(), d_off.data_ptr(), n, max_len, d_out.data_ptr(), d_stats.data_ptr(), d_ws.data_ptr(), ws,
                                stream=stream, ag_wildcard=ag, max_mismatches=max_mm, b=b)
    torch.cuda.synchronize()
    wa.Index.check_batch(d_ws.data_ptr(), stream)
    rounds = 8 * pat
    stride = (n + 63) // 64 * 64  # (bench.py's offset of the staged pass's control words)
    h_off = (64 * 4 + 256 * 16 * 8 + 3 * stride * 4 + ((n * max_len) // 16 + 10) * 4 + 15) // 16 * 16
    hctl = d_ws[h_off:h_off + 4 * 8 * rounds].view(torch.int32).cpu().numpy().reshape(8, pat, 8)
    LAST.update(hctl=hctl.copy(), dense=int(hctl[:, :, 0].sum()), giants=int(hctl[:, :, 5].sum()))
    end = se_ws // 16 * 16
    recs = d_ws[end - rounds * 16:end].view(torch.int64).cpu().numpy().reshape(rounds, 2).sum(axis=0)
    print("%d reads of up to %d bases%s, se_verify_share = %d: dense items %d, giants %d, gather items %d, rode along %d, records of items / of units %s" % (
        n, max_len, ", random PBAT" if rpbat else ", G->A" if ag else "", idx.get_option("se_verify_share"), int(hctl[:, :, 0].sum()),
        int(hctl[:, :, 5].sum()), int(hctl[:, :, 1].sum()), int(hctl[:, :, 7].sum()), recs.tolist()))
    out = d_out.cpu().numpy().tobytes() + (d_conv.cpu().numpy().tobytes() if rpbat else b"")
    return out, d_stats.cpu().numpy().tolist(), int(hctl[:, :, 7].sum()), recs.tolist()


@pytest.mark.parametrize("m", SHARED)
def test_records_equal_the_oracle_and_the_ungrouped_verifier_under_every_schedule(wa, world, index_options, m):
    idx, pool = world["idx"], world["pools"][100]
    sel = batch_of(pool, m)
    reads, want = [pool["reads"][i] for i in sel], pool["want"][sel]
    assert 2000 < len(reads) < 3100 and (want["times"] > 0).mean() > 0.8
    bases, offsets = wa.pack_reads(reads)
    defaults = {name: idx.get_option(name) for name in NAMES}
    assert defaults["se_verify_share"] == 1
    first = None
    for sched in SCHEDULES:
        for share in (1, 0):
            index_options(idx, **dict({name: sched.get(name, defaults[name]) for name in NAMES}, se_verify_share=share))
            for again in range(2 if not sched else 1):  # the second call meets the slots, counters and cursors the first one left
                got, stats = idx.map_se_batch(bases, offsets, ag_wildcard=False, max_mismatches=6, b=5000)
                assert_best_equal(got, want, "m=%d %s share=%d call %d" % (m, sched, share, again))
                st = {k: int(stats[k]) for k in stats.dtype.names}
                first = st if first is None else first
                assert st == first, "statistics differ under %s, se_verify_share = %d: %s, first %s" % (sched, share, st, first)


@pytest.mark.parametrize("m", SHARED)
def test_items_ride_along_wherever_two_reads_name_one_region(wa, world, index_options, m):
    idx, pool = world["idx"], world["pools"][100]
    sel = batch_of(pool, m)
    reads = [pool["reads"][i] for i in sel]
    index_options(idx, se_verify_share=0)
    rec0, st0, rode0, recs0 = device_run(wa, idx, reads, 6)
    assert rode0 == 0  # (the record counters are cleared and kept only with the option on)
    index_options(idx, se_verify_share=1)
    rec1, st1, rode1, recs1 = device_run(wa, idx, reads, 6)
    assert rec1 == rec0 and st1 == st0
    assert recs1[0] > 0 and recs1[1] <= recs1[0]
    if m >= 2:
        assert rode1 > 0 and recs1[1] < recs1[0], "m = %d: no item rode along (%d), records of items / units %s" % (m, rode1, recs1)
    else:
        assert recs1[1] <= recs1[0]
    # every item a unit of its own: nothing rides along, the same records
    index_options(idx, se_share_cap=1)
    rec2, st2, rode2, recs2 = device_run(wa, idx, reads, 6)
    assert rec2 == rec0 and st2 == st0 and rode2 == 0 and recs2[0] == recs2[1] == recs1[0]
    # grouped and counted only: the same records and the same records of all items.  The order inside a bucket is the
    # order its items arrive in, and a run that meets a 64-place slice border at another place is cut differently: the
    # units' counters are bounded, not equal -- a border costs a run at most one more unit of its region's size
    index_options(idx, se_share_cap=0, se_verify_share=2)
    rec3, st3, rode3, recs3 = device_run(wa, idx, reads, 6)
    assert rec3 == rec0 and st3 == st0 and recs3[0] == recs1[0]
    assert recs3[1] <= recs3[0] and (rode3 > 0) == (rode1 > 0)
    n_items = LAST["dense"] + LAST["giants"]
    borders = n_items // 64 + 24  # (every (chunk, round) cuts its own order)
    assert abs(rode3 - rode1) <= borders and abs(recs3[1] - recs1[1]) <= borders * 5000


def test_two_streams_and_two_state_slots_group_too(wa, world, index_options, m=130):
    """se_heavy_chunk = 384: the heavy list in chunks on two streams with a state slot each -- items ride along in chunks
    of both slots, the records are those of the ungrouped verifier"""
    idx, pool = world["idx"], world["pools"][100]
    sel = batch_of(pool, m)
    reads = [pool["reads"][i] for i in sel]
    assert len(reads) <= 8 * 384
    index_options(idx, se_heavy_chunk=384, se_verify_share=0)
    rec0, st0, rode0, _ = device_run(wa, idx, reads, 6)
    chunks0 = [c for c in range(8) if LAST["hctl"][c].any()]
    assert rode0 == 0 and len(chunks0) >= 2, "the heavy reads fill %d chunk(s)" % len(chunks0)
    index_options(idx, se_verify_share=1)
    for again in range(2):
        rec1, st1, rode1, recs1 = device_run(wa, idx, reads, 6)
        assert rec1 == rec0 and st1 == st0
        per_chunk = LAST["hctl"][:, :, 7].sum(axis=1)
        assert per_chunk[0] > 0 and per_chunk[1] > 0, "items that rode along per chunk: %s" % per_chunk.tolist()
        assert int(per_chunk.sum()) == rode1 and 0 < recs1[1] < recs1[0]


def test_reads_of_150_bases_keep_the_ungrouped_verifier(wa, world, index_options):
    idx, pool = world["idx"], world["pools"][150]
    sel = batch_of(pool, 130)
    reads, want = [pool["reads"][i] for i in sel], pool["want"][sel]
    bases, offsets = wa.pack_reads(reads)
    stats = []
    for share in (1, 0):
        index_options(idx, se_verify_share=share)
        got, st = idx.map_se_batch(bases, offsets, ag_wildcard=False, max_mismatches=10, b=5000)
        assert_best_equal(got, want, "150 bases, share=%d" % share)
        stats.append({k: int(st[k]) for k in st.dtype.names})
    assert stats[0] == stats[1]
    index_options(idx, se_verify_share=1)
    assert device_run(wa, idx, reads, 10)[2] == 0  # nothing is grouped on this route
