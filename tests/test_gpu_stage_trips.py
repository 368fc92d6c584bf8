"""The staged heavy kernels (k_se_stage, k_pe_stage) on a "slot ladder" genome, against the oracle: slots of every size
class of the long-slot search on both strands -- the first fence round of such a slot starts from pivot keys fetched
beside the slot's entries (map_common.h probe_entries_first) -- under every schedule that changes how reads reach the
kernel.  Records are compared bit for bit (assert_best_equal), statistics between the schedules.

The genome (about 1.9 Mbp in three sequences, default dir_bits).  Seed pattern 3 cares about one base in three, and a
directory slot wants 24 code bits of one or two bits a character, so a family is N copies of a fixed 72-base motif of
its own (24 care characters of every seed shift), each followed by 52 random bases: its copies share a slot at seeds 0,
1 and 2 and hold N distinct keys.  Half of the copies are reverse-complemented, so a slot holds N / 2 entries on either
strand.  N = 5, 16, 17, 33, 255, 257, 600, 4,100 -- and 8,800, because the plan sh = 12 needs more than 16 x 256
entries in ONE strand's slot.  A read is handed to the heavy pass by a slot of more than 20 entries, so the small
classes can only be searched at a LATER seed of such a read: 16, 17 and 11 copies of the 600 family carry a string of
their own in the motif's bases that seed 1 (seed 2) cares about.  One family of 300 identical 130-mers gives equal runs
over pivots and dense regions.  test_the_reads_reach_every_plan proves this on the host, from the directory of the CPU
harness's index at the opened dir_bits (tests/stage_trips_harness.cpp): a read counts as heavy when a probe of seed 0
meets a long slot (pass 1 always probes seed 0, so the hand-over is certain), and the tally shows which plans the probes
of those reads start from -- for the later seeds that is reachability: a read may be finished before them, which is why
the reads carry substitutions.  A batch's light reads are unique background reads that pass 1 keeps (the host index has
no danger filter: the few it hands over on a filter hit are found with its own count), and every batch checks pass 1's own
count of handed-over reads against the number it is named for (the hand-out windows' edge cases depend on it)."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import refio
from test_harness_cpu import assert_best_equal

pytestmark = pytest.mark.gpu

MOTIF, SPACER = 72, 52
FAMILIES = [5, 16, 17, 33, 255, 257, 600, 4100, 8800]
SUBS = [(16, 2), (17, 2), (11, 0)]  # (copies, motif bases = this mod 3 replaced) inside the 600 family: seed 1, seed 1, seed 2
HEAVY_SIZES = [1, 63, 65, 129, 2500]
SCHEDULES = [{}, {"se_heavy_chunk": 320}, {"se_pipe": 0}, {"se_stage_occ": 3}, {"se_stage_occ": 4}, {"grid": 1}, {"grid": 3},
             {"se_carry": 0, "se_heavy_chunk": 320}]


def _rand(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def make_ladder(rng):
    """-> (sequences, copies): copies = list of (sequence number, start, family, reverse-complemented)"""
    units = []  # (family, text, rc)
    for N in FAMILIES:
        motif = _rand(rng, MOTIF)
        variants = [motif] * N
        if N == 600:
            at = 0
            for cnt, res in SUBS:
                own = _rand(rng, MOTIF)
                v = "".join(own[i] if i % 3 == res else motif[i] for i in range(MOTIF))
                for k in range(cnt):
                    variants[at + k] = v
                at += cnt
        for k in range(N):
            units.append((N, variants[k] + _rand(rng, SPACER), k % 2 == 1))
    same = _rand(rng, 130)
    for k in range(300):
        units.append((130, same + _rand(rng, 20), k % 2 == 1))
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
        seqs.append(("ladder%d" % s, "".join(parts)))
    return seqs, copies


def convert(rng, s, ag, rate=0.95):
    a, b = ("G", "A") if ag else ("C", "T")
    return "".join(b if (c == a and rng.random() < rate) else c for c in s)


def substitute(rng, s, k):
    s = list(s)
    for p in rng.sample(range(len(s)), k):
        s[p] = rng.choice([c for c in "ACGT" if c != s[p]])
    return "".join(s)


def read_from_copy(rng, seqs, copy, L, ag):
    """a read that meets the copy's motif at seed 0, 1 or 2, from either strand, converted, with 0 .. 3 substitutions"""
    s, pos, fam, rc = copy
    g = seqs[s][1]
    unit = (130 + 20) if fam == 130 else (MOTIF + SPACER)
    off = rng.choice([0, 1, 2])
    if rc:  # the motif's first base is the unit's last: the read is taken from the other strand
        end = pos + unit + off
        frag = refio.revcomp(g[end - L:end])
    else:
        frag = g[pos - off:pos - off + L]
    assert len(frag) == L
    if rng.random() < 0.15:
        frag = refio.revcomp(frag)  # (the read's other end leads: its seeds meet the spacer, the record is the same copy's)
    return substitute(rng, convert(rng, frag, ag), rng.choice([0, 1, 1, 2, 2, 3]))


@pytest.fixture(scope="module")
def wa():
    import walt_amd
    assert walt_amd.device_count() >= 1, "no HIP device: the walt_amd hot path has no CPU fallback"
    return walt_amd


@pytest.fixture(scope="module")
def plans_lib():
    so = os.path.join(refio.HERE, "build", "libstage_trips_harness.so")  # (beside refio's harness: a scratch directory may not allow mapping code)
    os.makedirs(os.path.dirname(so), exist_ok=True)
    csrc = os.path.join(refio.ROOT, "walt_amd", "csrc")
    subprocess.run(["g++", "-O2", "-fopenmp", "-shared", "-fPIC", "-std=c++17", "-Wno-unknown-pragmas", "-DWALT_SEEDPATTERN=3", "-o", so,
                    os.path.join(refio.HERE, "stage_trips_harness.cpp"), os.path.join(csrc, "host_index.cpp")], check=True, timeout=600)
    L = ctypes.CDLL(so)
    vp, u32, ci = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
    L.hh_index_new.argtypes = [u32, vp, ci]
    L.hh_index_new.restype = vp
    L.hh_index_add_strand.argtypes = [vp, ci, vp, u32, vp, vp, u32]
    L.hh_index_add_strand.restype = ctypes.c_long
    L.hh_index_free.argtypes = [vp]
    L.st_probe_plans.argtypes = [vp, vp, vp, u32, ci, vp, vp]
    return L


@pytest.fixture(scope="module")
def ladder(wa, scratch, plans_lib):
    rng = random.Random(20240)
    seqs, copies = make_ladder(rng)
    fa = os.path.join(scratch, "ladder.fa")
    with open(fa, "w") as f:
        for nm, s in seqs:
            f.write(">%s\n%s\n" % (nm, s))
    path = os.path.join(scratch, "ladder.dbindex")
    wa.makedb(fa, path, threads=8)
    db = refio.DbIndex(path)
    idx = wa.Index.open(path, device=0, strands=wa.STRANDS_ALL)
    h = plans_lib.hh_index_new(db.n_chrom, db.lengths.ctypes.data, idx.dir_bits)
    for s in range(4):
        assert plans_lib.hh_index_add_strand(h, s, db.genome[s].ctypes.data, db.genome_len, db.counter[s].ctypes.data,
                                             db.index[s].ctypes.data, db.index[s].size) >= 0

    def plans(reads, ag):
        """(flag per read: 1 heavy for certain, 2 perhaps, 0 no long slot; tally[strand][class]) -- stage_trips_harness.cpp st_probe_plans"""
        bases, offsets = refio.pack_reads(reads)
        per_read = np.zeros(2 * len(reads), dtype=np.uint32)
        tally = np.zeros(14, dtype=np.uint64)
        assert plans_lib.st_probe_plans(h, bases.ctypes.data, offsets.ctypes.data, len(reads), int(ag), per_read.ctypes.data,
                                        tally.ctypes.data) == 0
        return per_read[0::2].copy(), tally.reshape(2, 7)

    yield {"seqs": seqs, "copies": copies, "db": db, "idx": idx, "plans": plans}
    idx.close()
    plans_lib.hh_index_free(h)


_pools = {}


def pool(ladder, kind, ag):
    """reads of one length class and conversion, their heavy flags, plan tally and oracle records (computed once)"""
    key = (kind, ag)
    if key in _pools:
        return _pools[key]
    rng = random.Random(1000 * ["100", "150", "mixed"].index(kind) + int(ag))
    seqs, copies = ladder["seqs"], ladder["copies"]
    big = [c for c in copies if c[2] >= 255 or c[2] == 130]
    small = [c for c in copies if c[2] < 255 and c[2] != 130]
    sub = [c for c in copies if c[2] == 600]
    length = (lambda: 100) if kind == "100" else (lambda: 150) if kind == "150" else (lambda: rng.randrange(60, 201))
    reads = [read_from_copy(rng, seqs, rng.choice(big), length(), ag) for _ in range(4000)]
    reads += [read_from_copy(rng, seqs, c, length(), ag) for c in sub]  # every copy of the 600 family: its three sub-families too
    reads += [read_from_copy(rng, seqs, rng.choice(small), length(), ag) for _ in range(200)]
    n_family = len(reads)
    for _ in range(400):  # unique background
        nm, g = seqs[rng.randrange(3)]
        L = length()
        p = rng.choice([rng.randrange(0, 30000 - L), len(g) - 30000 + rng.randrange(0, 30000 - L)])
        frag = g[p:p + L]
        frag = refio.revcomp(frag) if rng.random() < 0.5 else frag
        reads.append(substitute(rng, convert(rng, frag, ag), rng.choice([0, 1, 2, 3])))
    order = list(range(len(reads)))
    rng.shuffle(order)
    reads = [reads[i] for i in order]
    background = np.array([i >= n_family for i in order])
    flag, tally = ladder["plans"](reads, ag)
    heavy = flag == 1  # a long slot at seed 0: pass 1 hands the read over for certain
    light = (flag == 0) & background  # unique reads: no long slot, no region of more than four candidates
    # ... but the host index has no danger filter, and pass 1 also hands a read over on a filter hit: such background reads
    # are found with pass 1's own count (by halving) and left out
    import walt_amd

    def handed_over(cand):
        if cand.size == 0 or device_heavy_count(walt_amd, ladder["idx"], *walt_amd.pack_reads([reads[i] for i in cand]), ag,
                                                10 if kind == "150" else 6) == 0:
            return []
        if cand.size == 1:
            return [int(cand[0])]
        return handed_over(cand[:cand.size // 2]) + handed_over(cand[cand.size // 2:])
    light[handed_over(np.flatnonzero(light))] = False
    max_mm = 10 if kind == "150" else 6
    want, work = refio.oracle_se(ladder["db"], reads, ag=ag, max_mm=max_mm, b=5000, threads=8)
    _pools[key] = {"reads": reads, "heavy": heavy, "light": light, "tally": tally, "want": want, "max_mm": max_mm}
    return _pools[key]


def batch_of(p, n_heavy):
    """indexes of a batch with exactly n_heavy heavy reads, unique background reads mixed in (in pool order)"""
    hv = np.flatnonzero(p["heavy"])
    lt = np.flatnonzero(p["light"])
    assert hv.size >= n_heavy, "the pool holds %d heavy reads" % hv.size
    n_light = min(lt.size, max(3, n_heavy // 5))
    return np.sort(np.concatenate([hv[:n_heavy], lt[:n_light]]))


def device_control_words(wa, idx, bases, offsets, ag, max_mm):
    """the 64 control words at the start of the workspace after one call of the device form: [56] the reads pass 1
    handed to the heavy pass, [32] the length of the deferred list at the end of the call"""
    import torch
    dev = torch.device("cuda:0")
    n = offsets.size - 1
    max_len = int((offsets[1:] - offsets[:-1]).max())
    d_bases = torch.from_numpy(bases).to(dev)
    d_off = torch.from_numpy(offsets.astype(np.int64)).to(dev)
    d_out = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    d_stats = torch.zeros(4, dtype=torch.int64, device=dev)
    d_ws = torch.empty(wa.lib().walt_se_workspace_bytes(n, max_len), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    idx.map_se_batch_device(d_bases.data_ptr(), d_off.data_ptr(), n, max_len, d_out.data_ptr(), d_stats.data_ptr(), d_ws.data_ptr(),
                            d_ws.numel(), stream=stream, ag_wildcard=ag, max_mismatches=max_mm, b=5000)
    torch.cuda.synchronize()
    return d_ws[:64 * 4].view(torch.int32).cpu().numpy()


def device_heavy_count(wa, idx, bases, offsets, ag, max_mm):
    """reads pass 1 handed to the heavy pass in one call of the device form"""
    return int(device_control_words(wa, idx, bases, offsets, ag, max_mm)[56])


@pytest.mark.parametrize("ag", [False, True], ids=["CT", "GA"])
@pytest.mark.parametrize("kind", ["100", "150", "mixed"])
def test_the_reads_reach_every_plan(ladder, kind, ag):
    """host proof: among the probes the staged kernel can come to search, every class of first plan, on both strands"""
    p = pool(ladder, kind, ag)
    assert int(p["heavy"].sum()) >= 2500 and int(p["light"].sum()) >= 300
    names = ["1..4 entries", "sh 0, fewer than 16 pivots", "sh 0, 16 pivots", "sh 4", "sh 8", "sh 12", "sh 16"]
    for fi, strand in enumerate("+-"):
        for c in (0, 1, 3, 4, 5):
            assert p["tally"][fi][c] > 0, "%s %s: no probe of a heavy read starts from '%s' on strand %s (%s)" % (
                kind, "GA" if ag else "CT", names[c], strand, p["tally"][fi].tolist())
    mapped = p["want"]["times"] > 0
    assert mapped.mean() > 0.8 and (p["want"]["strand"] == b"-").any() and (p["want"]["strand"] == b"+").any()


@pytest.mark.parametrize("ag", [False, True], ids=["CT", "GA"])
@pytest.mark.parametrize("kind", ["100", "150", "mixed"])
@pytest.mark.parametrize("n_heavy", HEAVY_SIZES)
def test_stage_records_equal_oracle_under_every_schedule(wa, ladder, index_options, kind, ag, n_heavy):
    p = pool(ladder, kind, ag)
    sel = batch_of(p, n_heavy)
    reads = [p["reads"][i] for i in sel]
    want = p["want"][sel]
    bases, offsets = wa.pack_reads(reads)
    idx = ladder["idx"]
    names = ("se_heavy_chunk", "se_pipe", "se_stage_occ", "grid", "se_carry")
    defaults = {name: idx.get_option(name) for name in names}
    # the batch holds the heavy reads it is named for: pass 1's own count (device form: control word 56 of the workspace,
    # as bench.py reads it) -- the window-edge cases (63, 65, 129) depend on it
    assert device_heavy_count(wa, idx, bases, offsets, ag, p["max_mm"]) == n_heavy
    first = None
    for sched in SCHEDULES:
        index_options(idx, **{name: sched.get(name, defaults[name]) for name in names})
        got, stats = idx.map_se_batch(bases, offsets, ag_wildcard=ag, max_mismatches=p["max_mm"], b=5000)
        assert_best_equal(got, want, "%s %s heavy=%d %s" % (kind, "GA" if ag else "CT", n_heavy, sched))
        st = {k: int(stats[k]) for k in stats.dtype.names}
        if first is None:
            first = st
        assert st == first, "statistics differ under %s: %s, default schedule %s" % (sched, st, first)


DEFER_SCHEDULES = [{}, {"se_heavy_chunk": 64}, {"se_pipe": 0, "se_heavy_chunk": 64}, {"se_lit_side": 0, "se_heavy_chunk": 64},
                   {"se_carry": 0, "se_heavy_chunk": 64}]


@pytest.fixture(scope="module")
def crowded(wa, scratch):
    """The "crowded" genome of tests/test_gpu_parity.py::test_gpu_pe_small_heaps_with_overflow_list -- 300 short
    sequences cut from one 600-base unit plus the unit three times over: chromosome ends everywhere make probes
    dangerous, the repeats make slots long -- and 512 converted 100-base reads of it per conversion, with the oracle's
    records."""
    rng = random.Random(4242)
    unit = _rand(rng, 600)
    seqs = []
    for i in range(300):
        a = rng.randrange(0, 300)
        L = rng.choice([60, 90, 131, 150, 200, 260])
        s = list(unit[a:a + L])
        for _ in range(rng.randrange(0, 3)):
            s[rng.randrange(len(s))] = rng.choice("ACGT")
        seqs.append(("u%d" % i, "".join(s)))
    seqs.append(("long", unit * 3))
    fa = os.path.join(scratch, "crowded_se.fa")
    with open(fa, "w") as f:
        for nm, s in seqs:
            f.write(">%s\n%s\n" % (nm, s))
    path = os.path.join(scratch, "crowded_se.dbindex")
    wa.makedb(fa, path, threads=4)
    db = refio.DbIndex(path)
    idx = wa.Index.open(path, device=0, strands=wa.STRANDS_ALL)
    big = unit * 3
    sets = {}
    for ag in (False, True):
        reads = []
        for _ in range(512):
            a = rng.randrange(0, len(big) - 100)
            frag = big[a:a + 100]
            if rng.random() < 0.5:
                frag = refio.revcomp(frag)
            reads.append(substitute(rng, convert(rng, frag, ag), rng.choice([0, 1, 2])))
        want, work = refio.oracle_se(db, reads, ag=ag, max_mm=6, b=5000, threads=8)
        sets[ag] = {"reads": reads, "want": want, "too_short": int(work["too_short"])}
    yield {"idx": idx, "sets": sets}
    idx.close()


@pytest.mark.parametrize("ag", [False, True], ids=["CT", "GA"])
def test_side_launch_and_later_chunks_on_a_genome_that_defers(wa, crowded, index_options, ag):
    """Nothing that appends to the deferred list may run while the side launch's share of it is fixed (map_se.hip
    se_fork_literal): 512 reads that are heavy AND deferred, in eight chunks of the heavy list (se_heavy_chunk = 64 is
    applied up to 512 reads: four chunks per half when piped, eight in a row with se_pipe = 0), so that chunks behind
    the first pair still append when the snapshot is taken.  Records equal the oracle's under every schedule.
    Observed on the device (one call of the device form, default schedule): C->T reads 480 heavy and 393 deferred of 512,
    G->A reads 470 heavy and 393 deferred."""
    idx, p = crowded["idx"], crowded["sets"][ag]
    bases, offsets = wa.pack_reads(p["reads"])
    ctl = device_control_words(wa, idx, bases, offsets, ag, 6)
    heavy, deferred = int(ctl[56]), int(ctl[32])
    print("crowded %s: heavy %d, deferred %d of %d reads" % ("GA" if ag else "CT", heavy, deferred, len(p["reads"])))
    assert heavy >= 64, "pass 1 handed %d reads to the heavy pass: not every chunk holds reads" % heavy
    assert deferred >= 64, "%d reads were deferred" % deferred
    names = ("se_heavy_chunk", "se_pipe", "se_lit_side", "se_carry")
    defaults = {name: idx.get_option(name) for name in names}
    for sched in DEFER_SCHEDULES:
        index_options(idx, **{name: sched.get(name, defaults[name]) for name in names})
        got, stats = idx.map_se_batch(bases, offsets, ag_wildcard=ag, max_mismatches=6, b=5000)
        assert_best_equal(got, p["want"], "crowded %s %s" % ("GA" if ag else "CT", sched))
        assert int(stats["too_short"]) == p["too_short"], sched


@pytest.mark.parametrize("top_k", [5, 50])
def test_pe_stage_pairs_equal_oracle(wa, ladder, top_k):
    """1,200 pairs of the same genome through k_pe_stage (the shared resolve code)"""
    rng = random.Random(77)
    seqs, copies = ladder["seqs"], ladder["copies"]
    big = [c for c in copies if c[2] >= 255 or c[2] == 130]
    s1, s2 = [], []
    while len(s1) < 1200:
        s, pos, fam, rc = rng.choice(big) if rng.random() < 0.8 else rng.choice(copies)
        g = seqs[s][1]
        start = pos - rng.choice([0, 1, 2]) if not rc else pos - rng.randrange(40, 120)
        flen = rng.randrange(180, 400)
        if start < 0 or start + flen > len(g):
            continue
        frag = g[start:start + flen]
        if rng.random() < 0.5:
            frag = refio.revcomp(frag)
        s1.append(substitute(rng, convert(rng, frag[:100], False), rng.choice([0, 1, 2])))
        s2.append(substitute(rng, convert(rng, refio.revcomp(frag)[:100], True), rng.choice([0, 1, 2])))
    want, _, _ = refio.oracle_pe(ladder["db"], s1, s2, max_mm=6, b=5000, top_k=top_k, frag_range=1000, threads=8)
    res, _ = ladder["idx"].map_pe_batch(*wa.pack_reads(s1), *wa.pack_reads(s2), max_mismatches=6, b=5000, top_k=top_k, frag_range=1000)
    for f in ("best_times", "frag_len", "best_i", "best_j", "pair_mm"):
        assert np.array_equal(res[f], want[f]), (top_k, f)
    assert_best_equal(res["m1"], want["m1"], "pair m1 k=%d" % top_k)
    assert_best_equal(res["m2"], want["m2"], "pair m2 k=%d" % top_k)
    assert (want["best_times"] > 0).mean() > 0.5
