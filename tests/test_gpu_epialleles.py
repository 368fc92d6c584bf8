"""Four-CpG epiallele patterns per read on the GPU (include/walt_amd.h, "four-CpG epialleles"): walt_epialleles_* through
walt_amd.Epialleles, the composition with the calling (epi= on Index.meth_call_batch / Pileup.add_batch and their device
forms) and bin/walt -ME, all against one pure-Python restatement of the contract (epi_windows / expected_epi below), which
never uses the code under test: it finds the pairs by scanning the genome's text (find_pairs of the pair table's tests) and
takes every four calls that follow each other in a read."""
import bisect
import ctypes
import math
import os
import random
from fractions import Fraction

import numpy as np
import pytest

import refio
from test_gpu_cpgpairs import Hand, WALT_BIN, calls_at, expected_table, find_pairs, mode_args, run_walt, to_device
from test_gpu_meth_contigs import Genome, build_index, remove_index


# ---------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------
def epi_windows(calls):
    """calls: [(pair number, u)] of one read, the calls that have a pair, in read order -> [(entry, column)]"""
    out = []
    for t in range(len(calls) - 3):
        four = calls[t:t + 4]
        for s in (1, -1):
            if all(four[i][0] == four[0][0] + i * s for i in (1, 2, 3)):
                fwd = four if s == 1 else four[::-1]  # the lowest forward position first
                out.append((fwd[0][0], 8 * fwd[0][1] + 4 * fwd[1][1] + 2 * fwd[2][1] + fwd[3][1]))
    return out


def epi_walk(calls, numbers):
    """one read: calls (bytes), numbers[i] = the pair number of read position i or -1 -> [(entry, column)]"""
    return epi_windows([(numbers[i], 1 if b == 0x7A else 0) for i, b in enumerate(calls) if b in (0x7A, 0x5A) and numbers[i] >= 0])


def expected_epi(text, start_index, calls, offsets, pos, times, strand, skip=None, base=None, into=None):
    """count[n_pairs][16]; the arguments of expected_table (tests/test_gpu_cpgpairs.py)"""
    starts = [int(v) for v in start_index]
    genome_len = starts[-1]
    pairs = find_pairs(text, starts)
    number = {c: j for j, c in enumerate(pairs)}
    calls = np.asarray(calls, dtype=np.uint8)
    offsets = [int(v) for v in offsets]
    base = offsets[0] if base is None else base
    table = np.zeros((len(pairs), 16), dtype=np.uint64) if into is None else into
    for r in range(len(offsets) - 1):
        lo_b, hi_b = offsets[r] - base, offsets[r + 1] - base
        p = int(pos[r])
        if int(times[r]) != 1 or (skip is not None and int(skip[r]) != 0) or not 1 <= hi_b - lo_b <= 1024 or p >= genome_len:
            continue
        k = bisect.bisect_right(starts, p) - 1
        lo, hi = starts[k], starts[k + 1]
        minus = strand[r] in ("-", b"-")
        seen = []
        for i, b in enumerate(calls[lo_b:hi_b].tolist()):
            if b not in (0x7A, 0x5A):  # z, Z
                continue
            q = p + i
            if q >= hi:
                continue
            f = lo + hi - 1 - q if minus else q
            j = number.get(f, number.get(f - 1))
            if j is not None:
                seen.append((j, 1 if b == 0x7A else 0))
        for entry, column in epi_windows(seen):
            table[entry, column] += np.uint64(1)
    return table


def epi_sites_of(table, pairs, pos_lo=0, pos_hi=None, min_total=1):
    """the extraction of a table: [(pos, last, n0 .. n15)] of the entries with min_total reads and pos in [pos_lo, pos_hi)"""
    out = []
    for j in np.nonzero(np.asarray(table).sum(axis=1) >= min_total)[0].tolist():
        if pos_lo <= pairs[j] and (pos_hi is None or pairs[j] < pos_hi):
            out.append((pairs[j], pairs[j + 3]) + tuple(int(v) for v in table[j]))
    return out


def epi_list(sites):
    return [(int(s["pos"]), int(s["last"])) + tuple(int(v) for v in s["n"]) for s in sites]


def epi_stats(n):
    """(meth, epipoly, entropy, discordant) of sixteen counts, the first, second and fourth exactly"""
    total = sum(n)
    meth = Fraction(sum(c * (4 - bin(p).count("1")) for p, c in enumerate(n)), 4 * total)
    epipoly = 1 - sum(Fraction(c, total) ** 2 for c in n)
    entropy = -0.25 * math.fsum(c / total * math.log2(c / total) for c in n if c)
    return meth, epipoly, entropy, 1 - Fraction(n[0] + n[15], total)


def parse_epialleles(text):
    """-> [(chrom, pos, end, total, (n0 .. n15), (meth, epipoly, entropy, discordant))]"""
    out = []
    for line in text.splitlines():
        p = line.split("\t")
        assert len(p) == 24 and all(len(v.split(".")[1]) == 6 for v in p[20:]), line
        out.append((p[0], int(p[1]), int(p[2]), int(p[3]), tuple(int(v) for v in p[4:20]), tuple(float(v) for v in p[20:])))
    return out


def same_epialleles(got, want_rows):
    """want_rows: [(chrom, pos, end, n[16])]; integers exactly, the ratios to 1.5e-6 (the granularity of %.6f)"""
    assert [g[:3] for g in got] == [w[:3] for w in want_rows], (len(got), len(want_rows))
    for g, w in zip(got, want_rows):
        assert g[4] == tuple(w[3]) and g[3] == sum(w[3]), (g, w)
        for a, b in zip(g[5], epi_stats(w[3])):
            assert abs(a - float(b)) <= 1.5e-6, (g, w)


def epi_rows(table, pairs, names, starts, min_total=1):
    out = []
    for pos, last, *n in epi_sites_of(table, pairs, min_total=min_total):
        k = bisect.bisect_right(starts, pos) - 1
        assert last < starts[k + 1]
        out.append((names[k], pos - starts[k], last - starts[k], tuple(n)))
    return out


def tables_from_sam(sam_text, names, seqs):
    """The window table and the pair table a run's own SAM implies: unique records (no 0x4, 0x100, 0x200, 0x400) with an
    XM:Z: string, which is in the order of SEQ -- XM[k] lies on forward position POS - 1 + k -- walked forwards: a window
    does not depend on the direction its read is walked in."""
    text = "".join(seqs)
    starts = [0]
    for s in seqs:
        starts.append(starts[-1] + len(s))
    pairs = find_pairs(text, starts)
    calls, offsets, pos = [], [0], []
    for line in sam_text.splitlines():
        if line.startswith("@"):
            continue
        p = line.split("\t")
        xm = [t[5:] for t in p[11:] if t.startswith("XM:Z:")]
        if int(p[1]) & (0x4 | 0x100 | 0x200 | 0x400) or not xm:
            continue
        calls.append(xm[0])
        offsets.append(offsets[-1] + len(xm[0]))
        pos.append(starts[names.index(p[2])] + int(p[3]) - 1)
    flat = np.frombuffer("".join(calls).encode(), dtype=np.uint8)
    one, plus = [1] * len(pos), ["+"] * len(pos)
    return expected_epi(text, starts, flat, offsets, pos, one, plus), expected_table(text, starts, flat, offsets, pos, one, plus), pairs, starts


def dominated(epi, pair):
    """the contract's consequence: the windows of entry j with (u_i, u_i+1) = (a, b) are at most pairs[j + i][2 a + b]"""
    epi, pair = np.asarray(epi, dtype=np.uint64), np.asarray(pair, dtype=np.uint64)
    n = epi.shape[0]
    for i in range(3):
        for a in (0, 1):
            for b in (0, 1):
                cols = [p for p in range(16) if (p >> (3 - i)) & 1 == a and (p >> (2 - i)) & 1 == b]
                mine = epi[:, cols].sum(axis=1)
                theirs = np.zeros(n, dtype=np.uint64)
                theirs[:n - i] = pair[i:, 2 * a + b]
                if not (mine <= theirs).all():
                    return False
    return True


# ---------------------------------------------------------------------------
# the hand-made genome and its batches
# ---------------------------------------------------------------------------
# nine neighbouring pairs each (four for "g300"), no G between them: the distances between their C's
RULERS = {"g2": [2] * 8, "g5": [5] * 8, "g16": [16] * 8, "g40": [40] * 8, "g130": [130] * 7, "mixed": [2, 5, 16, 40, 130, 260, 390, 16],
          "g300": [300] * 3}


def epi_genome():
    """About 9,000 bases in 4 chromosomes.  Chromosome 0 holds the rulers and a CGCG.. stretch of 80 bases, then random
    sequence; chromosome 1 ends ..CGCGC and chromosome 2 starts GCGCGCG (no pair across the boundary, so no window either);
    chromosome 3 ends the genome with a pair; the starts are no multiples of 128."""
    rng = random.Random(2025)
    rnd = lambda n, al="ACGT": "".join(rng.choice(al) for _ in range(n))
    parts, at, where = [], 0, {}

    def put(s):
        nonlocal at
        parts.append(s)
        at += len(s)

    put(rnd(37, "ACT"))
    for name, gaps in RULERS.items():
        where[name] = at
        for d in gaps:
            put("CG" + rnd(d - 2, "ACT"))
        put("CG" + rnd(11, "ACT"))
    where["stretch"] = at
    put("CG" * 40)
    put(rnd(50, "ACT") + rnd(1500 + 77 - at % 128))
    c0 = "".join(parts)
    c1 = rnd(1490) + "ACGCGCGCGC"
    c2 = "GCGCGCG" + rnd(1600)
    c3 = rnd(800) + "TCGACGTTCGAACG"
    g = Genome(["e0", "e1", "e2", "e3"], [c0, c1, c2, c3])
    assert all(int(s) % 128 for s in g.start_index[1:])
    return g, where


def ruler_cs(where, name):
    cs = [where[name]]
    for d in RULERS[name]:
        cs.append(cs[-1] + d)
    return cs


def plus_read(cs, states, a=0, tail=3, blank=()):
    """(pos, calls) of a '+' record whose read position a lies on cs[0]: the C's of cs called with `states` (blank: members
    left '.')"""
    marks = {a + c - cs[0]: st for k, (c, st) in enumerate(zip(cs, states)) if k not in blank}
    return cs[0] - a, calls_at(a + cs[-1] - cs[0] + 1 + tail, marks)


def minus_read(g, chrom, cs, states, a=0, tail=3, blank=()):
    """the reverse-complement record of the same molecule: read position a lies on the G of cs[-1], the calls walk down"""
    lo, hi = int(g.start_index[chrom]), int(g.start_index[chrom + 1])
    top = cs[-1] + 1
    marks = {a + top - (c + 1): st for k, (c, st) in enumerate(zip(cs, states)) if k not in blank}
    return lo + hi - 1 - top - a, calls_at(a + top - (cs[0] + 1) + 1 + tail, marks)


def placement_cases(g, where):
    """chains of 4, 5 and 9 calls on every ruler (as far as 1,024 calls reach), on both strands, at read offsets that move
    the calls over slice and trip boundaries, behind lead reads of 0 .. 15 calls so that the reads sit at all 16 residues of
    the calls array's address -> (Hand, the windows these reads add)"""
    rng = random.Random(11)
    h, windows, k = Hand(), 0, 0
    for name in RULERS:
        cs_all = ruler_cs(where, name)
        for m in (4, 5, 9):
            if m > len(cs_all) or cs_all[m - 1] - cs_all[0] > 1000:
                continue
            for first in {0, len(cs_all) - m}:
                cs = cs_all[first:first + m]
                for a in (0, 3, 9, 14, 122, 127):
                    if a + cs[-1] - cs[0] + 5 > 1024 or cs[0] - a < 0:
                        continue
                    states = "".join(rng.choice("zZ") for _ in cs)
                    h.add(1, "+", calls_at(k % 16, {}))
                    k += 5
                    h.add(*((lambda pc: (pc[0], "+", pc[1]))(plus_read(cs, states, a))))
                    h.add(1, "+", calls_at(k % 16, {}))
                    k += 5
                    h.add(*((lambda pc: (pc[0], "-", pc[1]))(minus_read(g, 0, cs, states, a))))
                    windows += 2 * (m - 3)
    return h, windows


def edge_cases(g, where):
    """the contract's corner cases -> (Hand, the windows its first n_exact reads add, n_exact)"""
    h, windows = Hand(), 0
    st = where["stretch"]
    stretch = [st + 2 * k for k in range(40)]
    # the densest slice: CGCGCGCG x 2, eight calls in sixteen bases, then the whole stretch: 37 windows of 40 pairs
    for a in (0, 1, 15):
        h.add(*((lambda pc: (pc[0], "+", pc[1]))(plus_read(stretch[:8], "zZzzZZzZ", a))))
        windows += 5
    h.add(*((lambda pc: (pc[0], "+", pc[1]))(plus_read(stretch, "zZ" * 20, 5))))
    h.add(*((lambda pc: (pc[0], "-", pc[1]))(minus_read(g, 0, stretch, "zZ" * 20, 5))))
    windows += 2 * 37
    # a '.' on each of the four members of a chain of 7: what is left are chains of 6, 1 + 5, 2 + 4, 3 + 3
    cs = ruler_cs(where, "g16")[:7]
    for blank, left in ((0, 3), (1, 2), (2, 1), (3, 0)):
        h.add(*((lambda pc: (pc[0], "+", pc[1]))(plus_read(cs, "zzZzZZz", 2, blank=(blank,)))))
        h.add(*((lambda pc: (pc[0], "-", pc[1]))(minus_read(g, 0, cs, "zzZzZZz", 2, blank=(blank,)))))
        windows += 2 * left
    # a doubled call: the C and the G of one pair both called inside a chain of 8: 2 windows in front, 1 behind
    marks = {2 * k: "z" for k in range(8)}
    marks[9] = "Z"
    h.add(st, "+", calls_at(20, marks))
    windows += 2 + 1
    # calls on the G's of a '+' record, and the C of one pair with the G's of the next three
    h.add(st + 1, "+", calls_at(12, {0: "z", 2: "Z", 4: "z", 6: "Z"}))
    h.add(st, "+", calls_at(12, {0: "z", 3: "Z", 5: "z", 7: "Z"}))
    windows += 2
    # a z on a non-CpG position is ignored and does not break the chain; three calls are no window
    cs5 = ruler_cs(where, "g5")
    h.add(cs5[0], "+", calls_at(20, {0: "z", 2: "z", 5: "Z", 10: "z", 15: "Z"}))
    windows += 1
    h.add(cs5[0], "+", calls_at(20, {0: "z", 5: "Z", 10: "z"}))
    # a read of exactly 1,024 calls: the first four and the last four pairs it reaches of "g130"
    cs130 = ruler_cs(where, "g130")
    pos, body = plus_read(cs130, "zZzZzzZZ", 100, tail=1024 - 100 - 910 - 1)
    assert len(body) == 1024
    h.add(pos, "+", body)
    windows += 5
    # times 0 and 2 add nothing
    h.add(st, "+", b"z." * 8, times=0)
    h.add(st, "+", b"z." * 8, times=2)
    n_exact = len(h.pos)
    # the chromosome ends: ..CGCGC | GCGCGCG: four pairs at the end of chromosome 1 (one window), three at the start of
    # chromosome 2 (none), and no pair across; a read over the boundary stops calling at the end of its chromosome
    end1 = int(g.start_index[2])
    h.add(end1 - 12, "+", b"z" * 30)
    h.add(end1 - 9, "+", b".Z.z.Z.zZ")
    h.add(end1, "+", b"z" * 12)
    h.add(end1 - 5, "+", calls_at(14, {0: "z", 2: "z", 4: "z", 6: "z", 8: "z"}))
    # the pairs that end the genome
    h.add(g.genome_len - 300, "+", b"z" * 300)
    h.add(5, "-", b"Z" * 300)
    return h, windows, n_exact


def want_of(h, g, skip=None, into=None):
    calls, offsets, _ = h.arrays()
    return expected_epi(g.text, g.start_index, calls, offsets, h.pos, h.times, h.strand, skip, into=into)


def random_reads(g, rng, n, dense):
    """records anywhere in the genome (also across chromosome ends), both strands; dense: most reference CpGs called"""
    h = Hand()
    al = "zZ" * 6 + "xXhH." if dense else "zZ" * 3 + "...xhHU#A"
    for _ in range(n):
        L = rng.choice((1, 15, 16, 17, 31, 127, 128, 129, 1024, 40, 100, 150, 300))
        h.add(rng.randrange(0, g.genome_len), rng.choice("+-"), "".join(rng.choice(al) for _ in range(L)), rng.choice([0, 1, 1, 1, 1, 2]))
    return h


pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def wa():
    import walt_amd
    assert walt_amd.device_count() >= 1, "no HIP device: the walt_amd hot path has no CPU fallback"
    return walt_amd


@pytest.fixture(scope="module")
def small(wa, scratch):
    g, where = epi_genome()
    db, path, idx = build_index(g, scratch, "epialleles_small")
    try:
        yield {"g": g, "where": where, "idx": idx, "pairs": find_pairs(g.text, g.start_index)}
    finally:
        idx.close()
        remove_index(path)


# ---------------------------------------------------------------------------
# 1. hand-made adds and the extraction
# ---------------------------------------------------------------------------
def test_n_pairs_and_the_chromosome_boundary(wa, small):
    g, idx, pairs = small["g"], small["idx"], small["pairs"]
    assert 6000 < g.genome_len < 12000
    end1 = int(g.start_index[2])
    assert g.text[end1 - 5:end1] == "CGCGC" and g.text[end1] == "G" and end1 - 1 not in pairs and pairs[-1] == g.genome_len - 2
    ep, ap = idx.epialleles(), idx.cpg_pairs()
    assert ep.n_pairs == ap.n_pairs == len(pairs)
    assert ep.device_bytes >= 64 * len(pairs) + g.genome_len // 8 and ep.device_bytes - ap.device_bytes == 48 * len(pairs)
    assert ep.extract().size == 0
    # every C around the boundary called, and every G of the other strand: the window of the four pairs that end
    # chromosome 1, none from the three that start chromosome 2, none across
    h = Hand().add(end1 - 12, "+", calls_at(30, {k: "z" for k in range(3, 19, 2)})).add(end1, "+", calls_at(12, {1: "Z", 3: "Z", 5: "Z"}))
    lo, hi = int(g.start_index[1]), end1
    h.add(lo + hi - 1 - (end1 - 1), "-", calls_at(12, {1: "z", 3: "z", 5: "z", 7: "z"}))
    ep.add(*h.arrays())
    j = pairs.index(end1 - 9)
    assert pairs[j:j + 5] == [end1 - 9, end1 - 7, end1 - 5, end1 - 3, end1 + 1]
    got = epi_list(ep.extract(end1 - 40, end1 + 40))
    assert got == epi_sites_of(want_of(h, g), pairs, end1 - 40, end1 + 40) and [s[:2] for s in got] == [(end1 - 9, end1 - 3)]
    assert got[0][2 + 15] == 2 and sum(got[0][2:]) == 2
    ep.close()
    ap.close()


def test_hand_made_calls_host_form(wa, small):
    g, idx, pairs = small["g"], small["idx"], small["pairs"]
    hp, n_windows = placement_cases(g, small["where"])
    calls, offsets, rec = hp.arrays()
    assert {int(offsets[k]) % 16 for k in range(1, len(hp.pos), 2)} == set(range(16)) and max(len(c) for c in hp.calls) > 900
    want = want_of(hp, g)
    assert int(want.sum()) == n_windows > 300
    ep = idx.epialleles()
    ep.add(calls, offsets, rec)
    assert epi_list(ep.extract()) == epi_sites_of(want, pairs)
    # a '-' record and its reverse complement add to the same entry and column: every count is even
    assert (want % np.uint64(2) == 0).all()
    he, n_edge, n_exact = edge_cases(g, small["where"])
    assert int(want_of(he.head(n_exact), g).sum()) == n_edge
    want = want_of(he, g, into=want)
    assert int(want.sum()) > n_windows + n_edge
    ep.add(*he.arrays())
    got = ep.extract()
    assert epi_list(got) == epi_sites_of(want, pairs) and (want.sum(axis=0) > 0).all()  # every column is reached
    assert all(0 < int(s["last"]) - int(s["pos"]) <= 1023 for s in got) and max(int(s["last"]) - int(s["pos"]) for s in got) == 900
    # random reads, sparse and dense, on top; offsets that do not start at 0; skip bytes at stride 2; records at stride 64
    rng = random.Random(5)
    for dense in (False, True):
        hr = random_reads(g, rng, 700, dense)
        calls, offsets, rec = hr.arrays(64)
        skip = np.full((len(hr.pos), 2), 9, dtype=np.uint8)
        skip[:, 1] = [rng.choice([0, 0, 0, 1, 200]) for _ in hr.pos]
        before = int(want.sum())
        want = want_of(hr, g, skip[:, 1], into=want)
        assert int(want.sum()) > before + 50
        ep.add(calls, offsets + np.uint64(12345), rec, skip=skip[:, 1])
        assert epi_list(ep.extract()) == epi_sites_of(want, pairs), dense
    # n = 0; the host form rejects a read of 1025 calls and adds nothing of that batch; refusals name their cause
    ep.add(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64), Hand().arrays()[2])
    st = small["where"]["stretch"]
    with pytest.raises(wa.WaltError) as ei:
        ep.add(*Hand().add(st, "+", b"z." * 20).add(st, "+", b"z." * 512 + b"z").arrays())
    assert ei.value.code == wa.WALT_EINVAL and "1024" in str(ei.value)
    L = wa.lib()
    one, off, rec = Hand().add(st, "+", b"z.z.z.z.").arrays()
    for args, word in (((ep.handle, one.ctypes.data, off.ctypes.data, 1, rec.ctypes.data, 12, None, 1), "stride 12"),
                       ((ep.handle, one.ctypes.data, off.ctypes.data, 1, rec.ctypes.data, 16, one.ctypes.data, 0), "skip stride 0"),
                       ((ep.handle, one.ctypes.data, None, 1, rec.ctypes.data, 16, None, 1), "null"),
                       ((None, one.ctypes.data, off.ctypes.data, 1, rec.ctypes.data, 16, None, 1), "null epiallele table")):
        assert L.walt_epialleles_batch(*args) == wa.WALT_EINVAL and word in L.walt_last_error().decode(), word
    assert epi_list(ep.extract()) == epi_sites_of(want, pairs)
    ep.clear()
    assert ep.extract().size == 0 and ep.n_pairs == len(pairs)
    ep.close()


def test_device_form_alignments_strides_and_a_read_of_1025(wa, small):
    import torch
    g, idx, pairs = small["g"], small["idx"], small["pairs"]
    st = small["where"]["stretch"]
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    ep = idx.epialleles()
    h = placement_cases(g, small["where"])[0]
    he = edge_cases(g, small["where"])[0]
    for k in range(len(he.pos)):
        h.add(he.pos[k], he.strand[k], he.calls[k], he.times[k])
    # a read of more than 1,024 calls between counted reads adds nothing, its neighbours everything; a record whose
    # position lies at or behind the genome's end adds nothing
    h.add(st, "+", b"z." * 20).add(st, "+", b"z." * 512 + b"z").add(st + 2, "+", b"Z." * 20)
    h.add(g.genome_len, "+", b"z." * 20).add(0xFFFFFFF0, "-", b"z." * 20)
    rng = random.Random(6)
    hr = random_reads(g, rng, 300, True)
    for k in range(len(hr.pos)):
        h.add(hr.pos[k], hr.strand[k], hr.calls[k], hr.times[k])
    want = want_of(h, g)
    assert int(want.sum()) > 800
    for shift in range(16):
        stride = 64 if shift % 3 == 0 else 16
        calls, offsets, rec = h.arrays(stride)
        keep, d_calls, d_off, d_rec, s = to_device(torch, dev, calls, offsets, rec, shift)
        assert s == stride
        torch.cuda.synchronize()
        ep.clear()
        ep.add_device(d_calls, d_off.data_ptr(), len(h.pos), d_rec.data_ptr(), stride, stream=stream.cuda_stream)
        stream.synchronize()
        assert epi_list(ep.extract()) == epi_sites_of(want, pairs), (shift, stride)
    # skip bytes at stride 2 on the device, the null stream
    skip = np.full((len(h.pos), 2), 1, dtype=np.uint8)
    skip[:, 0] = [rng.choice([0, 0, 3]) for _ in h.pos]
    d_skip = torch.from_numpy(skip).to(dev)
    torch.cuda.synchronize()
    ep.clear()
    ep.add_device(d_calls, d_off.data_ptr(), len(h.pos), d_rec.data_ptr(), stride, d_skip.data_ptr(), 2)
    assert epi_list(ep.extract()) == epi_sites_of(want_of(h, g, skip[:, 0]), pairs)
    # n = 0 with null arrays is fine; refusals
    ep.add_device(None, None, 0, None)
    for args, kw, word in (((d_calls, d_off.data_ptr(), 1, d_rec.data_ptr()), dict(record_stride=8), "stride 8"),
                           ((d_calls, d_off.data_ptr(), 1, d_rec.data_ptr()), dict(skip_stride=0, d_skip=d_skip.data_ptr()), "skip stride 0"),
                           ((d_calls, d_off.data_ptr() + 4, 1, d_rec.data_ptr()), {}, "aligned"),
                           ((d_calls, d_off.data_ptr(), 1, d_rec.data_ptr() + 2), {}, "aligned"),
                           ((None, d_off.data_ptr(), 1, d_rec.data_ptr()), {}, "null"), ((d_calls, d_off.data_ptr(), 1, None), {}, "null")):
        with pytest.raises(wa.WaltError) as ei:
            ep.add_device(*args, **kw)
        assert ei.value.code == wa.WALT_EINVAL and word in str(ei.value), word
    ep.close()


def test_50000_copies_and_the_reverse_complement_record(wa, small):
    g, idx, pairs = small["g"], small["idx"], small["pairs"]
    cs = ruler_cs(small["where"], "g16")
    j = pairs.index(cs[0])
    assert pairs[j:j + 9] == cs
    ep = idx.epialleles()
    n = 50000
    states = "zZZzzZzzZ"
    pos, read = plus_read(cs, states, 7)
    h = Hand()
    h.pos, h.strand, h.times, h.calls = [pos] * n, ["+"] * n, [1] * n, [read] * n
    ep.add(*h.arrays())
    u = [1 if s == "z" else 0 for s in states]
    column = lambda k: 8 * u[k] + 4 * u[k + 1] + 2 * u[k + 2] + u[k + 3]
    expect = lambda copies: [(cs[k], cs[k + 3]) + tuple(copies if p == column(k) else 0 for p in range(16)) for k in range(6)]
    assert epi_list(ep.extract()) == expect(n)
    # the reverse-complement record of the same molecule lands on the same six entries, one column each
    rc = Hand().add(*((lambda pc: (pc[0], "-", pc[1]))(minus_read(g, 0, cs, states, 4))))
    assert epi_sites_of(want_of(rc, g), pairs) == expect(1)
    ep.add(*rc.arrays())
    assert epi_list(ep.extract()) == expect(n + 1)
    ep.close()


def test_dominance_over_the_pair_table(wa, small):
    g, idx, pairs = small["g"], small["idx"], small["pairs"]
    rng = random.Random(12)
    ep, ap = idx.epialleles(), idx.cpg_pairs()
    total = 0
    for dense in (True, False, True):
        h = random_reads(g, rng, 900, dense)
        ep.add(*h.arrays())
        ap.add(*h.arrays())
    epi = np.zeros((len(pairs), 16), dtype=np.uint64)
    pair = np.zeros((len(pairs), 4), dtype=np.uint64)
    index = {c: j for j, c in enumerate(pairs)}
    for s in ep.extract():
        epi[index[int(s["pos"])]] = s["n"]
    for s in ap.extract():
        pair[index[int(s["pos"])]] = s["n"]
    total = int(epi.sum())
    assert total > 500 and dominated(epi, pair)
    broken = pair.copy()
    broken[int(np.nonzero(epi.sum(axis=1))[0][0])] = 0
    assert not dominated(epi, broken)  # (the check can fail)
    ep.close()
    ap.close()


@pytest.fixture(scope="module")
def filled(wa, small):
    g, idx = small["g"], small["idx"]
    ep = idx.epialleles()
    h = random_reads(g, random.Random(7), 1500, True)
    hp = placement_cases(g, small["where"])[0]
    for k in range(len(hp.pos)):
        h.add(hp.pos[k], hp.strand[k], hp.calls[k], hp.times[k])
    ep.add(*h.arrays())
    table = want_of(h, g)
    assert len(epi_sites_of(table, small["pairs"])) > 150
    yield ep, table
    ep.close()


def test_extraction_ranges_min_total_and_capacity(wa, small, filled):
    import torch
    g, pairs = small["g"], small["pairs"]
    ep, table = filled
    want = epi_sites_of(table, pairs)
    assert epi_list(ep.extract()) == want
    # last is the walk's: the C of the fourth pair
    assert all(pairs[pairs.index(s[0]) + 3] == s[1] for s in want)
    pos, last = max(want, key=lambda s: s[1] - s[0])[:2]
    assert last - pos > 300
    # membership goes by pos alone: a range that ends or starts inside a window
    assert epi_list(ep.extract(0, pos + 1)) == [s for s in want if s[0] <= pos]
    assert epi_list(ep.extract(pos + 1, g.genome_len)) == [s for s in want if s[0] > pos]
    assert epi_list(ep.extract(pos, last)) == [s for s in want if pos <= s[0] < last]
    assert epi_list(ep.extract(pos, pos + 2)) == [s for s in want if s[0] == pos] and len(epi_list(ep.extract(pos, pos + 2))) == 1
    for lo, hi in ((0, 0), (pos, pos), (g.genome_len, g.genome_len), (pos + 1, pos + 2)):  # empty, or no pair inside
        assert ep.extract(lo, hi).size == 0
    rng = random.Random(8)
    totals = sorted(sum(s[2:]) for s in want)
    assert totals[0] == 1 and totals[-1] > 4
    for _ in range(30):
        lo = rng.randrange(0, g.genome_len)
        hi = rng.randrange(lo, g.genome_len + 1)
        m = rng.choice([1, 2, 3, totals[len(totals) // 2]])
        assert epi_list(ep.extract(lo, hi, m)) == [s for s in want if lo <= s[0] < hi and sum(s[2:]) >= m], (lo, hi, m)
    # min_total: 1, 2, above every total, 0
    assert epi_list(ep.extract(min_total=1)) == want
    two = epi_list(ep.extract(min_total=2))
    assert two == epi_sites_of(table, pairs, min_total=2) and 0 < len(two) < len(want)
    assert ep.extract(min_total=totals[-1]).size >= 1 and ep.extract(min_total=totals[-1] + 1).size == 0
    assert ep.extract(min_total=2 ** 40).size == 0
    with pytest.raises(wa.WaltError) as ei:
        ep.extract(min_total=0)
    assert ei.value.code == wa.WALT_EINVAL and "min_total" in str(ei.value)
    # range errors
    for lo, hi in ((5, 4), (0, g.genome_len + 1)):
        with pytest.raises(wa.WaltError) as ei:
            ep.extract(lo, hi)
        assert ei.value.code == wa.WALT_EINVAL and "range" in str(ei.value)
    # cap too small, host form: WALT_EINVAL, *n_out set, nothing written
    L = wa.lib()
    buf = np.full(len(two) * 72, 0x55, dtype=np.uint8).view(wa.epiallele_site_dtype)
    n = ctypes.c_uint64(0)
    assert L.walt_epialleles_extract(ep.handle, 0, g.genome_len, 2, buf.ctypes.data, len(two) - 1, ctypes.byref(n)) == wa.WALT_EINVAL
    assert n.value == len(two) and "room for" in L.walt_last_error().decode() and (buf.view(np.uint8) == 0x55).all()
    assert L.walt_epialleles_extract(ep.handle, 0, g.genome_len, 2, buf.ctypes.data, len(two), ctypes.byref(n)) == 0
    assert epi_list(buf) == two
    # device form on a side stream: exact cap, then cap too small: *d_n_out > cap and nothing written
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    for cap in (len(two), len(two) - 1, 0):
        d_out = torch.full((len(two) * 72 + 8,), 0x55, dtype=torch.uint8, device=dev)
        d_n = torch.zeros(1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        ep.extract_device(0, g.genome_len, 2, d_out.data_ptr() if cap else None, cap, d_n.data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
        assert int(d_n.item()) == len(two)
        got = d_out.cpu().numpy()
        if cap == len(two):
            assert epi_list(got[:len(two) * 72].view(wa.epiallele_site_dtype)) == two and (got[len(two) * 72:] == 0x55).all()
        else:
            assert (got == 0x55).all()
    with pytest.raises(wa.WaltError) as ei:
        ep.extract_device(0, g.genome_len, 0, None, 0, d_n.data_ptr())
    assert ei.value.code == wa.WALT_EINVAL and "min_total" in str(ei.value)


@pytest.mark.parametrize("blocks", [1, 2, 7, 300, 65536])
def test_extraction_does_not_depend_on_the_launch_shape(small, filled, index_options, blocks):
    ep, table = filled
    g = small["g"]
    plain = ep.extract().tobytes()
    part = ep.extract(1234, g.genome_len - 777, 2).tobytes()
    index_options(small["idx"], pile_extract_blocks=blocks)
    assert ep.extract().tobytes() == plain and ep.extract(1234, g.genome_len - 777, 2).tobytes() == part
    assert epi_list(ep.extract()) == epi_sites_of(table, small["pairs"])


def test_two_streams_feed_one_table(wa, small):
    import torch
    g, idx, pairs = small["g"], small["idx"], small["pairs"]
    dev = torch.device("cuda", 0)
    ep = idx.epialleles()
    rng = random.Random(9)
    batches = [random_reads(g, rng, 400 + 37 * k, True) for k in range(2)]
    want = want_of(batches[1], g, into=want_of(batches[0], g))
    staged = [to_device(torch, dev, *b.arrays(), shift=5 * k) for k, b in enumerate(batches)]
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
    torch.cuda.synchronize()
    reps = 5
    for _ in range(reps):
        for k in range(2):
            _, d_calls, d_off, d_rec, _ = staged[k]
            ep.add_device(d_calls, d_off.data_ptr(), len(batches[k].pos), d_rec.data_ptr(), stream=streams[k].cuda_stream)
    for s in streams:
        s.synchronize()
    assert int(want.sum()) > 200 and epi_list(ep.extract()) == epi_sites_of(want * np.uint64(reps), pairs)
    ep.close()


# ---------------------------------------------------------------------------
# 2. the composition with the calling
# ---------------------------------------------------------------------------
from test_gpu_cpgpairs import g1, g1_all, g1_pairs  # noqa: E402,F401  (fixtures)


def g1_epi_want(g1, calls, offsets, rec, skip=None):
    db, _, names, seqs = g1
    text = "".join(seqs)
    table = expected_epi(text, db.start_index, calls, offsets, rec["genome_pos"], rec["times"], [bytes(s) for s in rec["strand"]], skip)
    return epi_sites_of(table, find_pairs(text, db.start_index))


def test_fused_call_host_form(wa, g1, g1_all, g1_pairs):
    (b1, o1, b2, o2), res, excl = g1_pairs
    n = res.size
    rng = np.random.default_rng(8)
    skip = (rng.integers(0, 4, size=n) == 0).astype(np.uint8)
    call_len = rng.integers(20, 101, size=n).astype(np.uint32)
    ep, ep2, ap, ap_plain = g1_all.epialleles(), g1_all.epialleles(), g1_all.cpg_pairs(), g1_all.cpg_pairs()
    # Pileup.add_batch(..., epi=ep) equals Epialleles.add on the calls it returns; both mates into one table; the calls,
    # the counts, the statistics, the pile-up and the pair table are what they are without epi=
    pile, plain_pile = g1_all.pileup(), g1_all.pileup()
    for bases, offs, mate, cv in ((b1, o1, "m1", "T"), (b2, o2, "m2", "A")):
        got = pile.add_batch(bases, offs, res[mate], cv, pairs=ap, epi=ep)
        plain = plain_pile.add_batch(bases, offs, res[mate], cv, pairs=ap_plain)
        for x, y in zip(got, plain):
            assert x.tobytes() == y.tobytes()
        ep2.add(got[0], offs, res[mate])
    assert pile.extract()[0].tobytes() == plain_pile.extract()[0].tobytes()
    assert ap.extract().tobytes() == ap_plain.extract().tobytes() and ap.extract().size > 300
    pile.close()
    plain_pile.close()
    both = ep.extract()
    assert both.tobytes() == ep2.extract().tobytes() and both.size > 100 and int(both["n"].sum()) > 300
    # without pairs=, with call_len, excl, trim5 / trim3 and skip: the table is the restatement's on those calls
    for kw in (dict(call_len=call_len), dict(excl=excl), dict(trim5=7, trim3=5), dict(skip=skip),
               dict(call_len=call_len, excl=excl, trim5=3, trim3=9, skip=skip)):
        ep.clear()
        calls, _, _ = g1_all.meth_call_batch(b2, o2, res["m2"], "A", epi=ep, **kw)
        want = g1_epi_want(g1, calls, o2, res["m2"], kw.get("skip"))
        assert epi_list(ep.extract()) == want and len(want) > 30, sorted(kw)
        plain = g1_all.meth_call_batch(b2, o2, res["m2"], "A", **kw)
        assert plain[0].tobytes() == calls.tobytes()
    # the caller's calls NULL: the host form counts from its device copy
    ep.clear()
    none = g1_all.meth_call_batch(b1, o1, res["m1"], "T", want_calls=False, want_counts=False, want_stats=False, epi=ep)
    assert none == (None, None, None)
    full = g1_all.meth_call_batch(b1, o1, res["m1"], "T")
    assert epi_list(ep.extract()) == g1_epi_want(g1, full[0], o1, res["m1"])
    # epi= is keyword-only: the positional orders are the ones they were
    with pytest.raises(TypeError):
        g1_all.meth_call_batch(b1, o1, res["m1"], "T", None, True, True, None, True, None, None, None, None, 0, 0, 0, ep)
    for t in (ep, ep2, ap, ap_plain):
        t.close()


def test_fused_call_device_form_and_refusals(wa, g1, g1_all, g1_pairs, small):
    import torch
    (b1, o1, b2, o2), res, excl = g1_pairs
    n = res.size
    dev = torch.device("cuda", 0)
    d_bases = torch.from_numpy(b2).to(dev)
    d_offs = torch.from_numpy(o2.view(np.int64)).to(dev)
    d_pairs = torch.from_numpy(res.view(np.uint8).reshape(n, 64)).to(dev)
    d_excl = torch.from_numpy(excl.view(np.int32)).to(dev)
    stream = torch.cuda.Stream(device=dev)
    ep = g1_all.epialleles()
    total = int(o2[-1])
    outs, tables = [], []
    for with_ep, with_ap in ((False, True), (True, True), (True, False)):
        d_calls = torch.full((total + 48,), 0x23, dtype=torch.uint8, device=dev)
        d_counts = torch.zeros((n, 16), dtype=torch.uint8, device=dev)
        d_stats = torch.zeros(9, dtype=torch.int64, device=dev)
        pile, ap = g1_all.pileup(), g1_all.cpg_pairs()
        ep.clear()
        torch.cuda.synchronize()
        pile.add_batch_device(d_bases.data_ptr(), d_offs.data_ptr(), n, d_pairs.data_ptr() + 16, 64, None, 1, "A", None,
                              d_calls.data_ptr() + 3, d_counts.data_ptr(), d_stats.data_ptr(), stream=stream.cuda_stream,
                              d_excl=d_excl.data_ptr(), trim5=2, trim3=4, pairs=ap if with_ap else None, epi=ep if with_ep else None)
        stream.synchronize()
        outs.append((d_calls.cpu().numpy(), d_counts.cpu().numpy(), d_stats.cpu().numpy(), pile.extract()[0].tobytes()))
        tables.append((ap.extract().tobytes(), ep.extract().tobytes()))
        pile.close()
        ap.close()
    for other in outs[1:]:
        for x, y in zip(outs[0], other):
            assert (x == y) if isinstance(x, bytes) else np.array_equal(x, y)
    assert tables[0][0] == tables[1][0] and len(tables[0][0]) > 0 and tables[2][0] == b"" and tables[0][1] == b""
    assert tables[1][1] == tables[2][1]
    calls = outs[1][0][3:3 + total]
    want = g1_epi_want(g1, calls, o2, res["m2"])
    assert epi_list(ep.extract()) == want and len(want) > 30
    # d_calls NULL with a table: refused, and the message says why; a table of another index
    with pytest.raises(wa.WaltError) as ei:
        g1_all.meth_call_batch_device(d_bases.data_ptr(), d_offs.data_ptr(), n, d_pairs.data_ptr() + 16, 64, None, 1, "A", None,
                                      None, None, None, epi=ep)
    assert ei.value.code == wa.WALT_EINVAL and "d_calls" in str(ei.value) and "counted from the calls" in str(ei.value)
    other = small["idx"].epialleles()
    with pytest.raises(wa.WaltError) as ei:
        g1_all.meth_call_batch(b2, o2, res["m2"], "A", epi=other)
    assert ei.value.code == wa.WALT_EINVAL and "another index" in str(ei.value)
    other.close()
    assert epi_list(ep.extract()) == want
    ep.close()
    # an index without the reference has no table
    bare = wa.Index.open(g1[1], device=0, strands=wa.STRANDS_CT)
    with pytest.raises(wa.WaltError) as ei:
        bare.epialleles()
    assert ei.value.code == wa.WALT_EINVAL and "reference" in str(ei.value)
    bare.close()


# ---------------------------------------------------------------------------
# 3. command line
# ---------------------------------------------------------------------------
def other_files(out):
    d, b = os.path.dirname(out), os.path.basename(out)
    return sorted(f[len(b):] for f in os.listdir(d) if f.startswith(b) and f[len(b):][:1] not in ("", "-") and f != b + ".epialleles")


# The fewest lines a run on g1's golden libraries must write: below what the walk over each run's own SAM counted when the
# test was written (r 2032, A 1107, pe 2402, P 2402, R 2546, RP 2402; seed pattern 5: 1843, 7: 1805; -MEN 3: r 208, pe 423),
# so that an empty or a thinned-out file does not pass.
MIN_ROWS = {"r": 1500, "A": 800, "pe": 1800, "P": 1800, "R": 1900, "RP": 1800, "sp": 1300, "r-n3": 150, "pe-n3": 300}


def check_run_against_its_sam(g1, out, min_rows, min_total=1):
    _, _, names, seqs = g1
    epi, pair, pairs, starts = tables_from_sam(open(out).read(), names, seqs)
    assert dominated(epi, pair)
    want = epi_rows(epi, pairs, names, starts, min_total)
    got = parse_epialleles(open(out + ".epialleles").read())
    print("epialleles rows of %s: %d (the walk: %d)" % (os.path.basename(out), len(got), len(want)))
    same_epialleles(got, want)
    assert len(got) >= min_rows
    return got


@pytest.mark.parametrize("mode", ["r", "A", "pe", "P", "R", "RP"])
def test_cli_every_mode_against_its_own_sam(wa, g1, scratch, mode):
    path = g1[1]
    out = os.path.join(scratch, "epialleles_cli_" + mode)
    base = ["-i", path] + mode_args(scratch, mode) + ["-a", "-u"]
    spelling = {"r": "-ME", "A": "-epialleles", "pe": "--epialleles"}.get(mode, "-ME")
    log = run_walt(base + ["-o", out, spelling, "-MA", "-M", "-sam", "-v"])
    got = check_run_against_its_sam(g1, out, MIN_ROWS[mode])
    assert "[walt_amd epialleles: %d entries, %d windows" % (len(got), sum(r[3] for r in got)) in log
    # .epialleles is absent without -ME, and every other output of the run with it is byte-identical
    run_walt(base + ["-o", out + "-plain", "-MA", "-M", "-sam"])
    assert not os.path.exists(out + "-plain.epialleles")
    assert other_files(out) == other_files(out + "-plain") and {".methstats", ".allelic"} <= set(other_files(out))
    for sfx in [""] + other_files(out):
        assert open(out + sfx, "rb").read() == open(out + "-plain" + sfx, "rb").read(), sfx
    # -ME alone is a consumer: the same table, no .methstats
    run_walt(base + ["-o", out + "-alone", "-ME"])
    assert open(out + "-alone.epialleles", "rb").read() == open(out + ".epialleles", "rb").read()
    assert not os.path.exists(out + "-alone.methstats") and not os.path.exists(out + "-alone.allelic")
    if mode in ("r", "pe"):
        # -MEN 3 against the filtered walk, on one device (the extraction's min_total) and through the host's merge
        run_walt(base + ["-o", out + "-n3", "-ME", "-MEN" if mode == "r" else "--epiallele-min-reads", "3", "-M", "-sam"])
        few = check_run_against_its_sam(g1, out + "-n3", MIN_ROWS[mode + "-n3"], min_total=3)
        assert few == [r for r in got if r[3] >= 3] and 0 < len(few) < len(got)
        # two shares of the batch on two tables (the same device twice), and small batches: the same files
        run_walt(base + ["-o", out + "-g00", "-ME", "-g", "0,0", "-N", "1000"])
        assert open(out + "-g00.epialleles", "rb").read() == open(out + ".epialleles", "rb").read()
        run_walt(base + ["-o", out + "-g00n3", "-ME", "-MEN", "3", "-g", "0,0", "-N", "700"])
        assert open(out + "-g00n3.epialleles", "rb").read() == open(out + "-n3.epialleles", "rb").read()
    if mode == "r":
        # two read files that share an output name: one table after another
        fq = mode_args(scratch, mode)[1]
        run_walt(["-i", path, "-r", fq + "," + fq, "-o", out + "-two," + out + "-two", "-ME"])
        assert open(out + "-two.epialleles").read() == 2 * open(out + ".epialleles").read()
        # -MEN without -ME is refused
        import subprocess
        pr = subprocess.run([WALT_BIN] + base + ["-o", out + "-bad", "-MEN", "3", "-MA"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                            text=True, timeout=60)
        assert pr.returncode != 0 and "-MEN" in pr.stdout and "-ME" in pr.stdout and not os.path.exists(out + "-bad.allelic")


@pytest.mark.parametrize("case", ["D", "NO", "C_I3", "F", "MA_MC_ML"])
def test_cli_options_act_through_the_calls(wa, g1, scratch, case):
    from test_gpu_dedup import doubled
    path = g1[1]
    f1, f2 = os.path.join(refio.GOLDEN, "pe_1.fastq"), os.path.join(refio.GOLDEN, "pe_2.fastq")
    extra = {"D": ["-D"], "NO": ["-NO"], "F": ["-F", "2"], "MA_MC_ML": ["-MA", "-MC", "-ML"]}.get(case)
    if case == "D":
        (_, f1), (_, f2) = doubled(scratch, "epialleles_D", [f1, f2])
    if case == "C_I3":
        args = refio.golden_meta()["cases"]["pe_clip_sam_au"]["args"]
        extra = ["-C", args[args.index("-C") + 1], "-I3", "3"]
        f1, f2 = os.path.join(refio.GOLDEN, "pe_clip_1.fastq"), os.path.join(refio.GOLDEN, "pe_clip_2.fastq")
    out = os.path.join(scratch, "epialleles_opt_" + case)
    base = ["-i", path, "-1", f1, "-2", f2, "-a", "-u", "-M", "-sam"]
    run_walt(base + ["-o", out, "-ME"] + extra)
    got = check_run_against_its_sam(g1, out, 800)  # (the walk's own counts: 1076 with -C -I3, 1673 with -F 2, 2338 and more for the others)
    # the other outputs are byte-identical to the same run without -ME
    run_walt(base + ["-o", out + "-plain"] + extra)
    assert other_files(out) == other_files(out + "-plain") and not os.path.exists(out + "-plain.epialleles")
    for sfx in [""] + other_files(out):
        assert open(out + sfx, "rb").read() == open(out + "-plain" + sfx, "rb").read(), sfx
    if case in ("D", "NO", "F"):  # the option takes windows away
        run_walt(base + ["-o", out + "-without", "-ME"])
        without = check_run_against_its_sam(g1, out + "-without", 1800)
        assert sum(r[3] for r in got) < sum(r[3] for r in without)
    if case == "MA_MC_ML":
        assert {".allelic", ".methcounts", ".levels"} <= set(other_files(out))


@pytest.mark.parametrize("pattern", [5, 7])
def test_cli_seed_patterns_5_and_7(wa, g1, scratch, pattern):
    binary = os.path.join(refio.ROOT, "walt_amd", "bin", "walt_sp%d" % pattern)
    path = os.path.join(scratch, "epialleles_g1_sp%d.dbindex" % pattern)
    old = wa.PATTERN
    wa.set_pattern(pattern)
    try:
        wa.makedb(os.path.join(refio.GOLDEN, "g1.fa"), path, threads=4)
    finally:
        wa.set_pattern(old)
    out = os.path.join(scratch, "epialleles_cli_sp%d" % pattern)
    run_walt(["-i", path, "-r", os.path.join(refio.GOLDEN, "sp_se_ct.fastq"), "-o", out, "-ME", "-M", "-sam"], binary=binary)
    check_run_against_its_sam(g1, out, MIN_ROWS["sp"])


def test_without_the_option_a_pair_table_run_writes_what_it_wrote(wa, g1, scratch):
    """a -MA run's output directory, byte for byte, against the hashes of the same run on the parent commit"""
    import hashlib
    d = os.path.join(scratch, "epialleles_parent_dir")
    os.makedirs(d, exist_ok=True)
    out = os.path.join(d, "run")
    run_walt(["-i", g1[1], "-1", os.path.join(refio.GOLDEN, "pe_1.fastq"), "-2", os.path.join(refio.GOLDEN, "pe_2.fastq"), "-a", "-u",
              "-o", out, "-MA", "-M", "-MC", "-sam"])
    got = {f: hashlib.sha256(open(os.path.join(d, f), "rb").read()).hexdigest() for f in sorted(os.listdir(d))}
    print("hashes of the -MA run:", got)
    assert got == PARENT_HASHES


# sha256 of what the parent commit's bin/walt wrote for the run above (the same index file, the same reads)
PARENT_HASHES = {
    "run": "4d00b0dd33a6bcf108bd62a11cd3ecd8a3e383efe7180b601fa47281cdd7b459",
    "run.allelic": "82404c1b6cd213a91f54fcaaec419f0c0558fc647877f830c0cb5f8334fee733",
    "run.mapstats": "d1e36b6de9650f4f17413351020003b2660c4bfe2eba197051135e10b65ca8aa",
    "run.methcounts": "d2fa5c880b1dd8949794f95b416db977cadfc7ab55ed58619ca003cd86972caf",
    "run.methstats": "f4326a2c66b67692791fd78b735d14c76c052b15d4d00da42c0c3c9f1d932bad",
}
